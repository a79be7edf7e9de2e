"""The window walk, edge by edge, in all five places where its loop stands (csrc/walk.hpp): walk_next / walk_contig (contig_coverage),
share_walk_kernel (contig_share_coverage), match_walk_kernel (match_reads), sample_scan_kernel (contig_sample_coverage) and
pile_scan_kernel (pileup) -- at k = 20 .. 127, on graphs whose steps take every branch of cov_step (tests/test_walk_edges_host.py holds
the census and pins every expectation used here to the oracle, on a machine without a device).

The graph is the oracle's `-m 1` stream with the multiplicity of edge i set to i + 1 (walk_edges_ref.tagged_stream), so the per-window
coverage of the two contig calls IS the id + 1 of the edge the walk found.  The read scans give no id; there the 16 calls of match_reads,
call b with one contig per canonical edge number whose bit b is set, tell the edge of every hitting window up to strand, and the two
other scans are held to the same walk by their counters, per-edge counts and placements.

Then `denovo` consumes the validity bits of the graphs at k = 31 and 64 (thousands of edges the walks step from and land on), and
every call must answer as before: the walk does not look at those bits."""
import numpy as np
import pytest

from tests import walk_edges_ref as X

pytestmark = pytest.mark.gpu
_LUT = np.zeros(256, np.uint8)
_LUT[[ord(c) for c in X.DNA]] = [0, 1, 2, 3]


@pytest.fixture(scope="module")
def ctx():
    from megagta_amd import api
    c = api.Context(0)
    yield c
    c.close()


def make_world(ctx, oracle, k):
    from megagta_amd import api
    w = X.get(k, oracle)
    if "cz" not in w:
        w["cz"] = X.census(w)
    g = api.Graph(ctx, X.tagged_stream(w["es"], api.EdgeStream), keep_multiplicity=True)
    return dict(w=w, k=k, g=g, ctx=ctx, cz=w["cz"], before={})


@pytest.fixture(scope="module", params=X.KS, ids=[f"k{k}" for k in X.KS])
def world(request, ctx, oracle):
    d = make_world(ctx, oracle, request.param)
    yield d
    d["g"].free()


# ---- the expectations, built once per k ------------------------------------------------------------------------------------------------
def contig_case(d):
    d = d["w"]                                                               # (kept with the inputs: two fixtures share them)
    if "contigs" not in d:
        w = d
        two = X.step_contigs(w)
        seqs = two + X.straddle_contigs(w, d["cz"]) + X.read_contigs(w)
        ids, off = X.expected_ids(w["edge_of"], d["k"], seqs)
        searched, walked = X.walk_counts(ids, off)
        d["contigs"] = dict(seqs=seqs, n_two=len(two), ids=ids, off=off, searched=int(searched.sum()), walked=int(walked.sum()))
    return d["contigs"]


def read_case(d):
    d = d["w"]
    if "walk_reads" not in d:
        w = d
        reads = X.walk_reads(w, d["cz"])
        d["walk_reads"] = dict(reads=reads, every=X.canon_contigs(w), by_bit=[X.canon_contigs(w, b) for b in range(16)],
                          want={rev: X.read_expectation(w, reads, rev) for rev in (False, True)})
    return d["walk_reads"]


# ---- the device calls ------------------------------------------------------------------------------------------------------------------
def run_contigs(d, batch=0, hash_bits=64, calls=("cov", "share")):
    """-> per call `name`: name = the per-window multiplicities, name_off, name_counts = (index searches, windows found by a step),
    name_batches"""
    g, ctx, seqs = d["g"], d["ctx"], contig_case(d)["seqs"]
    ctx.set_coverage_batch(batch)
    ctx.set_share_hash_bits(hash_bits)
    out = {}
    try:
        for name in calls:
            r = g.contig_coverage(seqs, per_window=True, abundance=False) if name == "cov" else g.contig_share_coverage(seqs, per_window=True)
            out.update({name: r["per_window"], name + "_off": r["window_offsets"], name + "_counts": (r["stats"]["n_index_searches"], r["stats"]["n_walked"]),
                        name + "_batches": r["stats"]["n_batches"]})
    finally:
        ctx.set_coverage_batch(0)
        ctx.set_share_hash_bits(64)
    return out


def upload(ctx, reads, reverse):
    from megagta_amd import readlib
    start = np.zeros(len(reads) + 1, dtype=np.uint64)
    np.cumsum([len(s) for s in reads], out=start[1:])
    flat = "".join(s[::-1] for s in reads) if reverse else "".join(reads)
    return ctx.upload_reads(readlib.pack_codes(_LUT[np.frombuffer(flat.encode(), np.uint8)]), start)


def run_reads(d, reverse):
    g, rc_ = d["g"], read_case(d)
    rd = upload(d["ctx"], rc_["reads"], reverse)
    try:
        m = [g.match_reads(rd, rc_["by_bit"][b], counts=True, reads_reversed=reverse) for b in range(16)]
        s = g.contig_sample_coverage(rd, [len(rc_["reads"])], rc_["every"], per_window=True, reads_reversed=reverse)
        p = g.pileup(rd, rc_["every"], per_read=True, reads_reversed=reverse)
    finally:
        rd.free()
    ss, ps = s["stats"], p["stats"]
    return dict(match_hits=np.stack([x["hit_windows"] for x in m]), match_bits=np.stack([x["bits"] for x in m]),
                match_counts=[(x["stats"]["n_read_windows"], x["stats"]["n_walked"], x["stats"]["n_index_searches"], x["stats"]["n_matched_reads"]) for x in m],
                sample_count=s["per_window_count"], sample_share=s["per_window_share"], sample_mass=s["mass"], sample_lib_hits=s["lib_hit_windows"],
                sample_counts=(ss["n_read_windows"], ss["n_read_walked"], ss["n_read_index_searches"], ss["n_hit_windows"], ss["n_covered"], ss["n_keys"]),
                pile_reads=p["reads"], pile_counts=p["counts"], pile_uniq=p["uniq"], pile_contigs=p["contigs"],
                pile_stats=(ps["n_read_windows"], ps["n_read_walked"], ps["n_read_index_searches"], ps["n_hit_windows"], ps["n_reads_placed"], ps["n_placements"]))


def result(d, name):
    """the answer of a group of calls on the graph as loaded, computed once"""
    if name not in d["before"]:
        d["before"][name] = run_contigs(d) if name == "contigs" else run_reads(d, name == "stored_reversed")
    return d["before"][name]


NAMES = ("contigs", "stored_reversed", "stored_as_sequenced")


def same(a, b):
    assert a.keys() == b.keys()
    for key in a:
        if isinstance(a[key], np.ndarray):
            assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), key
        else:
            assert a[key] == b[key], key


# ---- 0. the device that shows the ids ----------------------------------------------------------------------------------------------------
def test_every_edge_carries_its_id(world):
    g, n = world["g"], world["w"]["og"].size
    assert g.size == n < 65535 and g.k == world["k"]
    assert np.array_equal(g.edge_multiplicity(np.arange(n)), np.arange(n) + 1)


# ---- 1. contig walks: exact ids ------------------------------------------------------------------------------------------------------------
def test_contig_walks_find_every_edge(world):
    w, cz, c = world["w"], world["cz"], contig_case(world)
    got = result(world, "contigs")
    ids, off = c["ids"], c["off"]
    assert np.array_equal(got["cov_off"], off) and np.array_equal(got["share_off"], off)
    print(f"k {world['k']}: {len(c['seqs'])} contigs, {ids.size} windows, {int((ids >= 0).sum())} with an edge, searched {c['searched']} walked {c['walked']}")
    # window 0 of label(e) + W(e) + c is e itself (no edge where e hangs on a tip node: the index search never answers one), window 1 the
    # edge the census found -- the expectation says so before the device is asked
    tip = w["ref"].tip[cz["e"]]
    first = np.repeat(np.where(tip, -1, cz["e"]), 4)
    assert np.array_equal(ids[0:2 * c["n_two"]:2], first) and not tip.all()
    stepped = ids[1:2 * c["n_two"]:2]
    assert np.array_equal(stepped, cz["found"].ravel())
    for name in ("cov", "share"):
        bad = np.nonzero(got[name].astype(np.int64) != ids + 1)[0]
        if bad.size:                                                          # name the step: (k, e, c) and the branches it takes
            i = int(np.searchsorted(off, bad[0], "right") - 1)
            where = f"contig {i} window {int(bad[0] - off[i])} of {c['seqs'][i]}"
            if i < c["n_two"]:
                j = i // 4
                where += (f": e {int(cz['e'][j])} c {X.DNA[i % 4]} hint_miss {bool(cz['hint_miss'][j])} straddle {bool(cz['straddle'][j, i % 4])} "
                          f"final {bool(cz['final'][j])} invalid {bool(cz['invalid'][j])} minus {bool(cz['minus'][j])}")
            raise AssertionError(f"{name} k {world['k']}: {bad.size} windows on a wrong edge; first {where}: got {int(got[name][bad[0]]) - 1} want {int(ids[bad[0]])}")
    assert got["cov_counts"] == got["share_counts"] == (c["searched"], c["walked"])


@pytest.mark.parametrize("how", ["cov_batch_1000", "share_batch_1000", "hash_bits_3"])
def test_contig_walks_do_not_depend_on_batch_or_table(world, how):
    """batches of 1 000 windows (hundreds per call; one call per case, the batches are most of its time) and a count table that keeps 3
    bits of its hash: the same ids, the same counts"""
    before = result(world, "contigs")
    if how == "hash_bits_3":
        got = run_contigs(world, hash_bits=3)
    else:
        got = run_contigs(world, batch=1000, calls=(how.split("_")[0],))
        assert all(got[key] > 100 for key in got if key.endswith("_batches"))
    for key in got:
        if not key.endswith("_batches"):
            same({key: before[key]}, {key: got[key]})


# ---- 2. read walks -------------------------------------------------------------------------------------------------------------------------
def check_reads(world, got, reverse):
    w, r = world["w"], read_case(world)
    want, reads = r["want"][reverse], r["reads"]
    n_windows = sum(max(0, len(s) - world["k"]) for s in reads)
    assert want["windows"] == n_windows
    # match_reads: call b holds one contig per canonical number with bit b set
    numbers = sorted(set(w["canon"].values()))
    assert len(numbers) == len(r["every"]) and 1 <= numbers[0] and numbers[-1] < 65536      # any two differ in one of the 16 bits
    for b in range(16):
        assert np.array_equal(got["match_hits"][b], want["hits"][b]), b
        assert np.array_equal(got["match_bits"][b], want["hits"][b] > 0), b
        assert got["match_counts"][b] == (n_windows, want["walked"], want["searched"], int((want["hits"][b] > 0).sum())), b
    ones = np.array([bin(c).count("1") if c > 0 else 0 for c in want["canon"].tolist()], np.int64)
    per_read = np.bincount(np.repeat(np.arange(len(reads)), np.diff(want["off"])), weights=ones, minlength=len(reads)).astype(np.int64)
    assert np.array_equal(got["match_hits"].astype(np.int64).sum(axis=0), per_read) and per_read.sum() > 10000
    # contig_sample_coverage: one library, one contig per canonical number -- every window with an edge hits
    n_found = int(want["found"].sum())
    assert np.array_equal(got["sample_count"][:, 0], X.window_counts(w, r["every"], reads, reverse))
    assert int(got["sample_lib_hits"][0]) == n_found == got["sample_counts"][3]
    assert got["sample_counts"][:3] == (n_windows, want["walked"], want["searched"])
    # pileup: the same contigs; a read is placed exactly when one of its windows hits
    assert got["pile_stats"][:4] == (n_windows, want["walked"], want["searched"], n_found)
    assert np.array_equal(got["pile_reads"]["n_placed"] > 0, want["found"] > 0)
    assert got["pile_stats"][4] == int((want["found"] > 0).sum())
    print(f"k {world['k']} reverse {reverse}: {len(reads)} reads, {n_windows} windows, {n_found} with an edge, walked {want['walked']} searched {want['searched']}")


@pytest.mark.parametrize("order", ["stored_reversed", "stored_as_sequenced"])
def test_read_walks_find_every_edge(world, order):
    check_reads(world, result(world, order), order == "stored_reversed")


# ---- 3. the validity bits are not looked at --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=X.DENOVO_KS, ids=[f"k{k}" for k in X.DENOVO_KS])
def consumed(request, ctx, oracle):
    """a tagged graph of its own: every answer as loaded, then `denovo` consumes the validity bits as the oracle's does"""
    d = make_world(ctx, oracle, request.param)
    try:
        for name in NAMES:
            result(d, name)
        g, w = d["g"], d["w"]
        bits, words = X.invalid_after_denovo(w, oracle)
        assert int((bits & ~w["ref"].invalid).sum()) > 100
        assert np.array_equal(g.invalid_bits(), w["og"].bitvectors()["invalid"])
        g.denovo(150, False, 0)
        assert np.array_equal(g.invalid_bits(), words)
        yield d
    finally:
        d["g"].free()


@pytest.mark.parametrize("name", NAMES)
def test_walks_do_not_look_at_validity_bits(consumed, name):
    got = run_contigs(consumed) if name == "contigs" else run_reads(consumed, name == "stored_reversed")
    same(consumed["before"][name], got)
