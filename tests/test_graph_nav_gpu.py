"""Every navigation primitive of the device graph, asked directly (mgta_sdbg_navigate) and compared exactly with the numpy restatement
of tests/graph_nav_ref.py, which tests/test_graph_nav_host.py pins to the oracle and to the reference's own probe files."""
import os

import numpy as np
import pytest

from tests import graph_nav_ref as R
from tests import helpers as H

pytestmark = pytest.mark.gpu

CHUNK = 1 << 18


@pytest.fixture(scope="module")
def ctx():
    from megagta_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _nav(g, op, a0, a1=None, a2=None):
    """Graph.navigate in chunks (the out_fd answer is 29 values per tuple)"""
    a0 = np.asarray(a0, np.int64)
    part = lambda a, lo: a if a is None or np.ndim(a) == 0 else np.asarray(a)[lo:lo + CHUNK]
    res = [g.navigate(op, a0[lo:lo + CHUNK], part(a1, lo), part(a2, lo)) for lo in range(0, max(a0.size, 1), CHUNK)]
    return np.concatenate(res)


def _sample(size, n, seed):
    """a seeded sample of about n edges plus the first and the last 3 000; every edge of a graph that is no larger"""
    if size <= n + 6000:
        return np.arange(size, dtype=np.int64)
    rng = np.random.default_rng(seed)
    return np.unique(np.concatenate([np.arange(3000), rng.integers(0, size, n), np.arange(size - 3000, size)])).astype(np.int64)


def _check_rank_select(g, ref):
    """every legal position and rank: -1, size - 1, total - 1 and total among them"""
    pos = np.arange(-1, ref.size, dtype=np.int64)
    assert np.array_equal(_nav(g, "rank_last", pos), ref.rank_last(pos))
    assert np.array_equal(_nav(g, "rank_tip", pos[1:]), ref.rank_tip(pos[1:]))
    r = np.arange(-1, ref.total_last + 1, dtype=np.int64)
    assert np.array_equal(_nav(g, "select_last", r), ref.select_last(r))
    for c in range(1, 5):
        assert np.array_equal(_nav(g, "rank_w", pos, c), ref.rank_w(c, pos)), c
        r = np.arange(-1, ref.total_w[c] + 1, dtype=np.int64)
        assert np.array_equal(_nav(g, "select_w", r, c), ref.select_w(c, r)), c
    # the symbol given per tuple, all four mixed in one call
    cs = (np.arange(pos.size) & 3) + 1
    assert np.array_equal(_nav(g, "rank_w", pos, cs), ref.rank_w(cs, pos))


def _check_chain(g, ref, e, deep):
    """3e: out_fd(e, none) is the restated OutgoingEdges with labels and multi1, each returned descriptor its restatement (all 29 columns:
    the n-th of g_out_nth_fd is the n-th of g_out_all_fd, `edge` untouched for n >= degree); then, two levels deep from the edges
    `deep`, for every returned (child, descriptor): out_fd(child, descriptor) == out_fd(child, none) == the restatement"""
    got = _nav(g, "out_fd", e, 0, -1)
    want = ref.out_fd(e)
    assert np.array_equal(got, want), ("out_fd(none)", e[np.nonzero((got != want).any(axis=1))[0][:5]].tolist())
    plain = ref.outgoing(e)                                                  # (its unused slots read -1, the chain leaves them alone)
    plain[:, 1:][plain[:, 1:] == -1] = R.UNTOUCHED
    assert np.array_equal(got[:, :5], plain)
    got = got[np.searchsorted(e, deep)]
    n_handed = 0
    for level in (1, 2):
        kids = [np.stack([got[:, 1 + j] >> 4, got[:, 5 + j], got[:, 9 + j]], axis=1)[(got[:, 0] > j) & (got[:, 9 + j] >= 0)] for j in range(4)]
        kids = np.unique(np.concatenate(kids), axis=0)
        if kids.shape[0] == 0:
            break
        n_handed += kids.shape[0]
        handed = _nav(g, "out_fd", kids[:, 0], kids[:, 1], kids[:, 2])
        own = _nav(g, "out_fd", kids[:, 0], 0, -1)
        assert np.array_equal(handed, own), (level, kids[np.nonzero((handed != own).any(axis=1))[0][:5]].tolist())
        assert np.array_equal(own, ref.out_fd(kids[:, 0])), level
        got = own
    # a hint that is one, two or three lines early (the look-up walks forwards from it) changes nothing
    v = deep[~ref.invalid[deep]]
    r, h = ref.fd_r(v), ref.hint(v)
    base = ref.out_fd(v)
    for early in (1, 2, 3):
        assert np.array_equal(_nav(g, "out_fd", v, r, np.maximum(h - early, 0)), base), early
    return n_handed


def _check_edges(g, ref, e, per_edge):
    """the operations that take an edge id, on the edges `e`; the ones restated edge by edge in Python on `per_edge`"""
    assert np.array_equal(_nav(g, "forward", e), ref.forward(e))
    assert np.array_equal(_nav(g, "backward", e), ref.backward(e))
    assert np.array_equal(_nav(g, "last_index", e), ref.last_index(e))
    assert np.array_equal(_nav(g, "outgoing", e), ref.outgoing(e))
    s = per_edge
    assert np.array_equal(_nav(g, "label", s), ref.label(s))
    assert np.array_equal(_nav(g, "incoming", s), ref.incoming(s))
    assert np.array_equal(_nav(g, "reverse_complement", s), ref.reverse_complement(s))
    assert np.array_equal(_nav(g, "prev_simple", s), ref.prev_simple(s))
    assert np.array_equal(_nav(g, "next_simple", s), ref.next_simple(s))


def _check_graph(g, ref, n_sample, seed=1):
    """every operation on every edge; on graphs beyond some tens of thousands of edges the operations restated edge by edge in Python
    on a seeded sample of about n_sample edges plus the first and last 3 000, the levels of the chain on three times as many"""
    assert g.size == ref.size
    every = np.arange(ref.size, dtype=np.int64)
    _check_rank_select(g, ref)
    _check_edges(g, ref, every, _sample(ref.size, n_sample, seed))
    return _check_chain(g, ref, every, _sample(ref.size, 3 * n_sample, seed + 1))


def _resident(ctx, d):
    """the same graph read off the stream where a build of the device left it"""
    from megagta_amd import api
    ctx.build_sdbg(ctx.upload_reads(d["packed"], d["start"]), d["k"], collect=False)
    return api.Graph(ctx, None, d["k"])


# ---- a. the goldens ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged29", "ragged47", "toy44"])
def test_goldens(ctx, oracle, golden_dir, name):
    """ragged k = 29 / 47: every operation on every edge; toy k = 44: every edge for the vectorised operations, label / incoming /
    reverse complement / simple paths on a seeded sample of 20 000 edges plus the first and last 3 000; ragged k = 29 also from the
    device-resident stream"""
    from megagta_amd import api
    d = R.get_input(name, oracle, golden_dir)
    g = api.Graph(ctx, d["stream"].edges())
    n_handed = _check_graph(g, d["ref"], 10 ** 9 if name != "toy44" else 20000)
    assert n_handed > min(d["ref"].size, 60000)
    if name == "ragged29":
        _check_graph(_resident(ctx, d), d["ref"], 3000)


@pytest.mark.parametrize("case,k", [("ragged", 29), ("ragged", 47), ("toy", 44)])
def test_reference_probe_lines(ctx, oracle, golden_dir, case, k):
    """the reference binary's own answers, every column the device can be asked for: rank_last, rank_w 1..4, select_last, fwd, label,
    in-degree and in-edges, out-degree and out-edges; w and multi1 of a probed edge through the packed entry it has among the out-edges
    of an edge into its node"""
    from megagta_amd import api
    d = R.get_input(f"{case}{k}", oracle, golden_dir)
    g = api.Graph(ctx, d["stream"].edges())
    _, qs = H.parse_probe_graph(H.gz_lines(os.path.join(golden_dir, case, f"graph_k{k}.txt.gz")))
    e = np.array([q["e"] for q in qs], np.int64)
    assert _nav(g, "rank_last", e).tolist() == [q["rank_last"] for q in qs]
    for c in range(1, 5):
        assert _nav(g, "rank_w", e, c).tolist() == [q["rank_w"][c] for q in qs], c
    assert _nav(g, "select_last", np.array([q["rank_last"] - 1 for q in qs])).tolist() == [q["select_last"] for q in qs]
    out = _nav(g, "outgoing", e)
    assert out[:, 0].tolist() == [q["od"] for q in qs]
    assert [[x >> 4 for x in o[1:1 + max(o[0], 0)]] for o in out.tolist()] == [q["out"] for q in qs]
    full = [q for q in qs if "fwd" in q]
    ef = np.array([q["e"] for q in full], np.int64)
    fw, lab, inc = _nav(g, "forward", ef), _nav(g, "label", ef), _nav(g, "incoming", ef)
    assert [f for f, q in zip(fw.tolist(), full) if q["w"]] == [q["fwd"] for q in full if q["w"]]
    assert [f for f, q in zip(fw.tolist(), full) if not q["w"]] == [R.UNDEFINED for q in full if not q["w"]]
    assert ["".join("$ACGT"[c] for c in row) for row in lab] == [q["label"] for q in full]
    assert inc[:, 0].tolist() == [q["id"] for q in full]
    assert [o[1:1 + max(o[0], 0)] for o in inc.tolist()] == [q["in"] for q in full]
    seen = [(q, q["in"][0]) for q in full if q["valid"] and q["id"] > 0]
    assert len(seen) > 100
    back = _nav(g, "outgoing", np.array([p for _, p in seen]))
    for (q, p), o in zip(seen, back.tolist()):
        mine = [x for x in o[1:1 + o[0]] if x >> 4 == q["e"]]
        assert mine == [q["e"] << 4 | q["multi1"] << 3 | (q["w"] - 4 if q["w"] > 4 else q["w"])], (q["e"], p)


# ---- b. line and sample edges -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.GROUPS["b"])
def test_small_graphs(ctx, oracle, golden_dir, name):
    """one line (every `li + 1 < n_lines` guard), sizes 0 / 1 / 63 past a line boundary, select totals below, at and past one sample;
    k = 9 .. 95 (1 to 6 words per tip label): every operation on every edge"""
    from megagta_amd import api
    d = R.get_input(name, oracle, golden_dir)
    g = api.Graph(ctx, d["stream"].edges())
    _check_graph(g, d["ref"], 10 ** 9)
    if name == "size_129":
        _check_graph(_resident(ctx, d), d["ref"], 10 ** 9)


# ---- c. low complexity, tips, dense -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.GROUPS["c"])
def test_seeded_graphs(ctx, oracle, golden_dir, name):
    """a symbol absent over dozens of lines and poly-A reads; many tips; in- and out-degree 4 nearly everywhere at k = 9 (sampled for the
    edge-by-edge operations); the constructed fan whose hints lie up to four lines early"""
    from megagta_amd import api
    d = R.get_input(name, oracle, golden_dir)
    g = api.Graph(ctx, d["stream"].edges())
    _check_graph(g, d["ref"], 10 ** 9 if name != "dense" else 6000)
    if name == "tips":
        _check_graph(_resident(ctx, d), d["ref"], 10 ** 9)


# ---- d. arbitrary bit patterns: rank and select need no consistent graph ----------------------------------------------------------------
def test_rank_select_on_arbitrary_records(ctx):
    from megagta_amd import api
    rec, bucket_items = R.synthetic_records()
    s = api.EdgeStream(k=21, words_per_tip=2, bucket_items=bucket_items, records=rec, large=np.zeros(0, np.uint16),
                       tips=np.zeros(2 * int(((rec >> 5) & 1).sum()), np.uint32))
    g = api.Graph(ctx, s)
    _check_rank_select(g, R.NavRef.from_records(21, rec, bucket_items))


# ---- f. guards ----------------------------------------------------------------------------------------------------------------------
def test_guards(ctx, oracle, golden_dir):
    """null arguments, negative n, c = 0 and 5, ids = size, r = total + 1, a hint past the last line: MGTA_EINVAL with the outputs
    untouched; an empty graph answers without a launch; forward of a $ edge and backward of a tip read MGTA_NAV_UNDEFINED"""
    from megagta_amd import api
    d = R.get_input("ragged29", oracle, golden_dir)
    ref = d["ref"]
    g = api.Graph(ctx, d["stream"].edges())
    L, ops = ctx._L, api.Graph.NAV_OPS
    EINVAL = -1

    def raw(op, a0, a1=None, a2=None, n=None, handle=g.h, out="own", sym=None):
        a = [None if x is None else np.ascontiguousarray(x, dtype=np.int64) for x in (a0, a1, a2)]
        n = a[0].size if n is None else n
        buf = np.full(29 * max(n, 1), 77, np.int64)
        rc = L.mgta_sdbg_navigate(handle, ops[op], *[None if x is None else x.ctypes.data for x in a], n, None if out is None else buf.ctypes.data,
                                  None if sym is None else sym.ctypes.data)
        assert (buf == 77).all() or rc == 0, "a refused call wrote into its output"
        return rc
    assert raw("rank_last", [0]) == 0
    assert raw("rank_last", [0], handle=None) == EINVAL and raw("rank_last", None, n=1) == EINVAL and raw("rank_last", [0], out=None) == EINVAL
    assert raw("rank_w", [0]) == EINVAL and raw("select_w", [0]) == EINVAL and raw("out_fd", [0], [0]) == EINVAL       # a missing argument array
    assert raw("label", [0]) == EINVAL                                                                                  # no room for the symbols
    assert raw("rank_last", [0], n=-1) == EINVAL
    assert L.mgta_sdbg_navigate(g.h, 99, None, None, None, 0, None, None) == EINVAL
    for c in (0, 5):
        assert raw("rank_w", [0], [c]) == EINVAL and raw("select_w", [0], [c]) == EINVAL
    for op in ("rank_last", "rank_tip", "forward", "backward", "last_index", "outgoing", "incoming", "prev_simple", "next_simple", "reverse_complement"):
        assert raw(op, [0, ref.size]) == EINVAL and raw(op, [-2, 0]) == EINVAL, op
        assert raw(op, [0, ref.size - 1]) == 0, op
    assert raw("rank_tip", [-1]) == EINVAL and raw("forward", [-1]) == EINVAL and raw("rank_last", [-1]) == 0
    assert raw("rank_w", [ref.size], [1]) == EINVAL and raw("rank_w", [-2], [1]) == EINVAL
    assert raw("select_last", [ref.total_last + 1]) == EINVAL and raw("select_last", [-2]) == EINVAL and raw("select_last", [ref.total_last]) == 0
    for c in range(1, 5):
        assert raw("select_w", [ref.total_w[c] + 1], [c]) == EINVAL and raw("select_w", [ref.total_w[c]], [c]) == 0
    sym = np.zeros(2 * ref.k, np.uint8)
    assert raw("label", [0, ref.size], sym=sym) == EINVAL and not sym.any()
    assert raw("out_fd", [ref.size], [0], [-1]) == EINVAL and raw("out_fd", [0], [0], [ref.n_lines]) == EINVAL and raw("out_fd", [0], [0], [-2]) == EINVAL
    assert raw("rank_last", [], n=0) == 0
    with pytest.raises(api.MegaGtaError):
        g.navigate("forward", [ref.size])
    # a descriptor whose hint lies behind the bit it asks for is refused on the device, from the hint line's own rank
    v = np.nonzero(~ref.invalid & (ref.fd_r(np.arange(ref.size)) < ref.rank_last((ref.n_lines - 1) * 64 - 1)))[0][:50]
    assert v.size == 50 and (g.navigate("out_fd", v, ref.fd_r(v), ref.n_lines - 1)[:, 0] == R.UNDEFINED).all()
    # the values that stand for "undefined": read off, on the edges the graph holds anyway
    dollar, tips = np.nonzero(ref.W == 0)[0], np.nonzero(ref.tip)[0]
    assert dollar.size > 50 and tips.size > 50
    assert (g.navigate("forward", dollar) == api.Graph.NAV_UNDEFINED).all() and (g.navigate("backward", tips) == api.Graph.NAV_UNDEFINED).all()
    assert api.Graph.NAV_UNDEFINED == R.UNDEFINED and api.Graph.NAV_UNTOUCHED == R.UNTOUCHED
    # an empty graph: rank of -1, select of -1 and of 0 = total are the tuples in range
    empty = api.Graph(ctx, api.EdgeStream(k=29, words_per_tip=2, bucket_items=np.zeros(65536, np.int64), records=np.zeros(0, np.uint16),
                                          large=np.zeros(0, np.uint16), tips=np.zeros(0, np.uint32)))
    assert empty.navigate("rank_last", [-1]).tolist() == [0] and empty.navigate("rank_w", [-1], 3).tolist() == [0]
    assert empty.navigate("select_last", [-1, 0]).tolist() == [-1, 0] and empty.navigate("select_w", [-1, 0], 2).tolist() == [-1, 0]
    for op in ("rank_last", "forward", "outgoing", "rank_tip"):
        assert raw(op, [0], handle=empty.h) == EINVAL, op
    assert raw("select_last", [1], handle=empty.h) == EINVAL
