"""CPU only: the numpy restatement of the graph's navigation (tests/graph_nav_ref.py), which tests/test_graph_nav_gpu.py holds the device
to, is itself pinned here -- to the oracle's C calls, to the reference binary's own probe files -- and the inputs of the device tests
are shown to take the hard paths of the forward-descriptor chain."""
import os

import numpy as np
import pytest

from tests import graph_nav_ref as R
from tests import helpers as H


def _edges_to_check(name, size):
    if name != "toy44":
        return np.arange(size, dtype=np.int64)
    rng = np.random.default_rng(44)
    return np.unique(np.concatenate([np.arange(3000), rng.integers(0, size, 6000), np.arange(size - 3000, size)])).astype(np.int64)


@pytest.mark.parametrize("name", ["ragged29", "ragged47", "toy44"])
def test_restatement_equals_the_oracle(oracle, golden_dir, name):
    """every operation on every edge of ragged k = 29 / 47 (a sample of toy k = 44), and every legal position and rank of rank / select"""
    d = R.get_input(name, oracle, golden_dir)
    og, ref = d["og"], d["ref"]
    e = _edges_to_check(name, og.size)
    el = e.tolist()
    pos = np.concatenate([[-1], e])
    assert ref.rank_last(pos).tolist() == [og.rank_last(p) for p in pos.tolist()]
    assert (ref.total_last, [ref.total_w[c] for c in range(1, 5)]) == R._totals(og)
    assert ref.rank_f == [og.rank_last(x - 1) for x in og.f.tolist()]
    r = np.arange(-1, ref.total_last + 1) if name != "toy44" else np.concatenate([[-1], np.arange(0, ref.total_last, 37), [ref.total_last - 1, ref.total_last]])
    assert ref.select_last(r).tolist() == [og.select_last(x) for x in r.tolist()]
    for c in range(1, 5):
        assert ref.rank_w(c, pos).tolist() == [og.rank_w(c, p) for p in pos.tolist()], c
        r = np.arange(-1, ref.total_w[c] + 1) if name != "toy44" else np.concatenate([[-1], np.arange(0, ref.total_w[c], 37), [ref.total_w[c] - 1, ref.total_w[c]]])
        assert ref.select_w(c, r).tolist() == [og.select_w(c, x) for x in r.tolist()], c
    fw, bw, li = ref.forward(e), ref.backward(e), ref.last_index(e)
    nxt, last_l = [og.size] * (og.size + 1), ref.last.tolist()                  # GetLastIndex by a scan from the end
    for y in range(og.size - 1, -1, -1):
        nxt[y] = y if last_l[y] else nxt[y + 1]
    n_fw = n_bw = 0
    for x, f, b, l in zip(el, fw.tolist(), bw.tolist(), li.tolist()):
        if ref.W[x] != 0:                                                    # Forward is defined for an edge that carries a symbol
            assert f == og.forward(x), x
            n_fw += 1
        else:
            assert f == R.UNDEFINED
        if not ref.tip[x]:                                                   # Backward for an edge of a node that has an edge into it
            assert b == og.backward(x), x
            n_bw += 1
        else:
            assert b == R.UNDEFINED
        assert l == nxt[x], x
    assert n_fw > 0.9 * e.size and n_bw > 0.9 * e.size
    out, inc, lab = ref.outgoing(e, packed=False), ref.incoming(e), ref.label(e)
    packed = ref.outgoing(e)
    for i, x in enumerate(el):
        n, o = og.outgoing(x)
        assert out[i, 0] == n and out[i, 1:1 + max(n, 0)].tolist() == o and (out[i, 1 + max(n, 0):] == -1).all(), x
        for j in range(max(n, 0)):                                           # the packed form: id << 4 | multi1 << 3 | label
            assert packed[i, 1 + j] == (o[j] << 4 | int(ref.multi1[o[j]]) << 3 | int(ref.lab[o[j]])), x
        n, o = og.incoming(x)
        assert inc[i, 0] == n and inc[i, 1:1 + max(n, 0)].tolist() == o, x
    step = 1 if name != "toy44" else 5
    for i in range(0, e.size, step):
        assert "".join("$ACGT"[c] for c in lab[i]) == og.label(el[i]), el[i]
    # the reverse complement through the oracle's index search; the simple-path steps through its IncomingEdges / OutgoingEdges
    sub = e if name != "toy44" else e[::3]
    rc, ps, ns = ref.reverse_complement(sub), ref.prev_simple(sub), ref.next_simple(sub)
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}

    def uniq(call, x):
        n, ids = call(x)
        return ids[0] if n == 1 else -1
    found = 0
    for x, a, p, nx in zip(sub.tolist(), rc.tolist(), ps.tolist(), ns.tolist()):
        if ref.invalid[x]:
            assert (a, p, nx) == (-1, -1, -1), x
            continue
        kmer = og.label(x) + "$ACGT"[ref.lab[x]]
        assert a == og.index_edge("".join(comp[ch] for ch in reversed(kmer))), x
        found += a >= 0
        q = uniq(og.incoming, x)
        assert p == (q if q != -1 and uniq(og.outgoing, q) != -1 else -1), x
        q = uniq(og.outgoing, x)
        assert nx == (q if q != -1 and uniq(og.incoming, q) != -1 else -1), x
    assert found > 0.9 * (~ref.invalid[sub]).sum() and (ps >= 0).sum() > 100 and (ns >= 0).sum() > 100


@pytest.mark.parametrize("case,k", [("ragged", 29), ("ragged", 47), ("toy", 44)])
def test_restatement_equals_the_reference_probe(oracle, golden_dir, case, k):
    """every column of the reference binary's probe lines that the device can answer"""
    ref = R.get_input(f"{case}{k}", oracle, golden_dir)["ref"]
    hdr, qs = H.parse_probe_graph(H.gz_lines(os.path.join(golden_dir, case, f"graph_k{k}.txt.gz")))
    assert ref.size == int(hdr["size"][0]) and ref.k == int(hdr["k"][0]) and ref.f == [int(x) for x in hdr["f"]]
    e = np.array([q["e"] for q in qs], np.int64)
    assert ref.W[e].tolist() == [q["w"] for q in qs]
    assert ref.last[e].tolist() == [q["last"] for q in qs] and ref.tip[e].tolist() == [q["tip"] for q in qs]
    assert (~ref.invalid[e]).tolist() == [q["valid"] for q in qs] and ref.multi1[e].tolist() == [q["multi1"] for q in qs]
    out = ref.outgoing(e, packed=False)
    assert out[:, 0].tolist() == [q["od"] for q in qs]
    assert [o[1:1 + max(o[0], 0)] for o in out.tolist()] == [q["out"] for q in qs]
    assert ref.rank_last(e).tolist() == [q["rank_last"] for q in qs]
    for c in range(1, 5):
        assert ref.rank_w(c, e).tolist() == [q["rank_w"][c] for q in qs], c
    assert ref.select_last(ref.rank_last(e) - 1).tolist() == [q["select_last"] for q in qs]
    full = [i for i, q in enumerate(qs) if "fwd" in q]
    assert len(full) > 100
    ef = e[full]
    fw, lab, inc = ref.forward(ef), ref.label(ef), ref.incoming(ef)
    for i, j in enumerate(full):
        q = qs[j]
        if q["w"] != 0:
            assert fw[i] == q["fwd"], q["e"]
        assert "".join("$ACGT"[c] for c in lab[i]) == q["label"], q["e"]
        assert inc[i, 0] == q["id"] and inc[i, 1:1 + max(q["id"], 0)].tolist() == q["in"], q["e"]


def test_rank_select_restated_on_records_that_are_no_graph():
    """the synthetic records of the device test: cumsum / nonzero against counting by hand, and the shapes the records promise"""
    rec, bucket_items = R.synthetic_records()
    ref = R.NavRef.from_records(21, rec, bucket_items)
    W, last = (rec & 15).tolist(), ((rec >> 4) & 1).tolist()
    for p in (-1, 0, 1, 63, 64, 65, 64 * 40 - 1, 64 * 90, ref.size - 2, ref.size - 1):
        assert ref.rank_last([p])[0] == sum(last[:p + 1])
        for c in range(1, 5):
            assert ref.rank_w(c, [p])[0] == sum(1 for w in W[:p + 1] if w == c)
    ones = [i for i, b in enumerate(last) if b]
    assert ref.select_last([-1, 0, 1, 63, 64, 65, len(ones) - 1, len(ones)]).tolist() == [-1] + [ones[i] for i in (0, 1, 63, 64, 65, len(ones) - 1)] + [ref.size]
    per_line = np.add.reduceat(ref.last.astype(int), np.arange(0, ref.size, 64))
    assert (per_line == 0).sum() >= 30 and (per_line[:-1] == 64).sum() >= 4
    assert (ref.pos_w[4] >> 6).tolist() == [0, 0, 0, ref.n_lines - 1, ref.n_lines - 1]
    walk = max(int(((p >> 6) - (p[np.arange(p.size) >> 6 << 6] >> 6)).max()) for p in [ref.pos_last] + [ref.pos_w[c] for c in range(1, 5)])
    assert walk >= 30, walk


def test_inputs_take_the_hard_paths(oracle, golden_dir, capsys):
    """Which paths of g_outset_from / g_fd_of / g_select_* the inputs of tests/test_graph_nav_gpu.py take, counted over every valid edge
    (NavRef.paths): (a) the target node lies in the target line, (b) it continues into the line before, (c) bit 63 of the line before is
    a last | tip bit, (d) the hint is one line early, (e) two or more lines early, (f) an a + 4 edge before the first plain a of its
    line, (g) lines Select walks from its sample.

    (e) in graphs of reads: a line's hint is the target line of the last plain a before the line; the target of the j-th plain a of
    the line lies j nodes further on, so two or more lines on only when the line holds dozens of plain a whose target nodes have
    several out-edges each.  None of the random, golden, low-complexity, tip-heavy or dense inputs has such a line (dense: of four
    nodes that differ in their first letter only one carries the plain a, so 64 edges hold at most 16).  A build CAN produce it, and
    the `fan` input does by construction (R.reads_fan)."""
    counts = {}
    for group, names in R.GROUPS.items():
        for name in names:
            counts[name] = R.get_input(name, oracle, golden_dir)["ref"].paths()
    with capsys.disabled():
        print()
        for name, p in counts.items():
            print(f"  paths {name:10s} edges {p['edges']:7d}  a {p['a']:7d}  b {p['b']:5d}  c {p['c']:6d}  d {p['d']:6d}  e {p['e']:3d}  f {p['f']:5d}  g {p['g']}")
    for group, names in R.GROUPS.items():
        for key in "abcdf":
            assert sum(counts[n][key] for n in names) > 0, (group, key)
    for name in R.GROUPS["a"] + ["dense"]:
        for key in "abcdf":
            assert counts[name][key] > 0, (name, key)
    assert counts["fan"]["e"] > 0
    assert max(counts["lowcomplex"]["g"][f"w{c}"] for c in range(1, 5)) >= 8
    # the sizes and totals the small graphs were grown to
    sizes = {n: R.get_input(n, oracle, golden_dir)["og"].size for n in R.SMALL}
    assert sizes["one_line"] < 64 and [sizes[f"size_{s}"] for s in (65, 127, 128, 129, 191, 192)] == [65, 127, 128, 129, 191, 192]
    assert R.get_input("last_64", oracle, golden_dir)["ref"].total_last == 64 and R.get_input("last_65", oracle, golden_dir)["ref"].total_last == 65
    assert 64 in R.get_input("w_64", oracle, golden_dir)["ref"].total_w.values() and 65 in R.get_input("w_65", oracle, golden_dir)["ref"].total_w.values()
    one = R.get_input("one_line", oracle, golden_dir)["ref"]
    assert one.total_last < 64 and max(one.total_w.values()) < 64
    assert {R.get_input(n, oracle, golden_dir)["ref"].wpt for n in R.SMALL} == {1, 2, 3, 4, 5, 6}      # k = 9, 21 / 32, 44, 64, 79, 95
    low, tips, dense = (R.get_input(n, oracle, golden_dir)["ref"] for n in ("lowcomplex", "tips", "dense"))
    assert (~low.multi1).sum() > 1000 and tips.tip.sum() > 200
    od = dense.outgoing(np.nonzero(~dense.invalid)[0])[:, 0]
    assert (od == 4).mean() > 0.5


def test_descriptor_chain_restated(oracle, golden_dir):
    """the restated step: a descriptor handed on gives what the edge's own line gives; a hint never lies behind its target (asserted in
    paths()); `none` exactly for an out-edge in the line before the target line"""
    for name in ("ragged29", "fan", "tips"):
        ref = R.get_input(name, oracle, golden_dir)["ref"]
        e = np.nonzero(~ref.invalid)[0]
        o = ref.out_fd(e)
        assert np.array_equal(o[:, :5], np.where(ref.outgoing(e) == -1, np.where(np.arange(5) == 0, -1, R.UNTOUCHED), ref.outgoing(e)))
        for j in range(4):
            has = o[:, 0] > j
            child = o[has, 1 + j] >> 4
            none = o[has, 9 + j] == -1
            assert np.array_equal(none, (child >> 6) != (ref.forward(e[has]) >> 6))
            again = ref.out_fd(child[~none], o[has, 5 + j][~none], o[has, 9 + j][~none])
            assert np.array_equal(again, ref.out_fd(child[~none]))
