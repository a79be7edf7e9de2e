"""Edge multiplicities on the device graph and per-contig coverage / abundance against the CPU oracle.

Expected values never come from the code under test:
    mult = records >> 8;  mult[mult == 255] = large                      (oracle.Stream.edges(), in stream = edge-id order)
    expected(window) = mult[index_edge(window)] if index_edge(window) >= 0 else 0      (oracle.Graph.index_edge)
and, as a second witness that does not go through the oracle's graph, a brute-force count in numpy on a reads-only `-m 1` graph:
the multiplicity of a (k+1)-mer is the number of windows equal to it over all reads and their reverse complements, capped at 65535
(k + 1 odd, so no window is its own reverse complement)."""
import os
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

from megagta_amd import coverage as cv
from megagta_amd import hmm as hmmlib
from megagta_amd import readlib, synth
from tests import helpers as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "megagta_amd", "bin", "megagta")
DRIVER = os.path.join(ROOT, "megagta_amd", "megagta.py")
DNA = "ACGT"
COMP = str.maketrans("ACGTacgt", "TGCAtgca")


def rc(s):
    return s.translate(COMP)[::-1]


@pytest.fixture(scope="module")
def ctx():
    from megagta_amd import api
    c = api.Context(0)
    yield c
    c.close()


def oracle_mult(es) -> np.ndarray:
    """full multiplicity of every edge from the oracle's stream"""
    m = (es.records >> 8).astype(np.int64)
    big = m == 255
    assert int(big.sum()) == es.large.size                              # the two counts agree
    m[big] = es.large
    return m


def expected_windows(og, mult, seq, k):
    """-> (coverage per window, edge id per window) from the oracle"""
    cov, ids = [], []
    for p in range(len(seq) - k):
        w = seq[p:p + k + 1].upper()
        e = og.index_edge(w) if set(w) <= set(DNA) else -1              # no N -> G folding: an N was never counted
        ids.append(e)
        cov.append(int(mult[e]) if e >= 0 else 0)
    return cov, ids


def check_call(res, seqs, k, want_cov):
    """the per-window values of a contig_coverage(per_window=True) result and its per-contig fields against want_cov (list of lists)"""
    pw, off, c = res["per_window"], res["window_offsets"], res["contigs"]
    assert off[-1] == sum(len(w) for w in want_cov) == res["stats"]["n_windows"]
    for i, (s, w) in enumerate(zip(seqs, want_cov)):
        assert len(w) == max(0, len(s) - k)
        assert pw[off[i]:off[i + 1]].tolist() == w, i
        r = cv.stats_of_windows(w, len(s))
        got = dict(len=int(c[i]["len"]), windows=int(c[i]["n_windows"]), covered=int(c[i]["n_covered"]), sum=int(c[i]["sum"]),
                   median=int(c[i]["median"]), min=int(c[i]["min"]), max=int(c[i]["max"]))
        assert got == r, (i, got, r)


# ---- 1. every edge, every load route ------------------------------------------------------------------------------------------------
def _build_inputs(case, golden_dir):
    if case == "toy":
        return readlib.load_for_build(os.path.join(golden_dir, "toy", "reads.lib")), 44, 1, False
    if case == "ragged":
        return readlib.load_for_build(os.path.join(golden_dir, "ragged", "reads.lib")), 29, 1, False
    return readlib.load_for_build(os.path.join(golden_dir, "toy", "reads.lib")), 44, 2, True      # -m 2 --need_mercy


@pytest.mark.parametrize("case", ["toy", "ragged", "toy_m2_mercy"])
def test_every_edge_multiplicity_through_all_load_routes(ctx, oracle, golden_dir, tmp_path, case):
    from megagta_amd import api
    (packed, start), k, m, mercy = _build_inputs(case, golden_dir)
    ost = oracle.Stream.build(packed, start, k, threads=4) if m == 1 else oracle.Stream.build_solid(packed, start, k, m, mercy, threads=4)
    oes = ost.edges()
    want = oracle_mult(oes)
    rd = ctx.upload_reads(packed, start)
    stream = ctx.build_sdbg(rd, k, min_count=m, need_mercy=mercy)
    assert stream.md5() == oes.md5()
    ids = np.arange(want.size)
    # host stream (records + large words through mgta_sdbg_load_large)
    g = api.Graph(ctx, stream, keep_multiplicity=True)
    assert g.size == want.size and np.array_equal(g.edge_multiplicity(ids), want)
    with pytest.raises(api.MegaGtaError, match=r"\(-1\)"):
        g.edge_multiplicity([g.size])                                     # an id out of range is an error
    with pytest.raises(api.MegaGtaError, match=r"\(-1\)"):
        g.edge_multiplicity([-1])
    g.free()
    # resident: the stream where the build left it
    ctx.build_sdbg(rd, k, min_count=m, need_mercy=mercy, collect=False)
    g = api.Graph(ctx, None, keep_multiplicity=True)                      # (no k given: the graph knows the build's)
    assert g.k == k and np.array_equal(g.edge_multiplicity(ids), want)
    r = g.contig_coverage(["ACGT" * 30, "AC"], per_window=True)          # buffers are sized by the graph's k, not by the caller's
    assert r["per_window"].size == 120 - k and r["window_offsets"].tolist() == [0, 120 - k, 120 - k]
    g.free()
    # files, 1 and 3 of them, in one range and in several
    for nf in (1, 3):
        prefix = str(tmp_path / f"{case}_{nf}")
        api.write_sdbg(prefix, stream, num_files=nf)
        for rng_records in (None, max(64, want.size // 5)):
            if rng_records:
                os.environ["MGTA_LOAD_RANGE_RECORDS"] = str(rng_records)
            try:
                g = api.Graph.from_files(ctx, prefix, keep_multiplicity=True)
            finally:
                os.environ.pop("MGTA_LOAD_RANGE_RECORDS", None)
            assert g.k == k and np.array_equal(g.edge_multiplicity(ids), want), (nf, rng_records)
            g.free()


def hot_reads(seed=21):
    """1500 reads of 100 bp from a random 5 kb genome, half of them reverse-complemented, + one 100 bp read 300 times"""
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, 5000)
    reads = []
    for i in range(1500):
        p = int(rng.integers(0, 5000 - 100 + 1))
        r = genome[p:p + 100]
        reads.append((3 - r)[::-1] if i % 2 else r)
    hot = rng.integers(0, 4, 100)
    reads += [hot] * 300
    return np.array(reads, dtype=np.uint8)


@pytest.fixture(scope="module")
def hot(ctx, oracle):
    from megagta_amd import api
    k = 30
    reads = hot_reads()
    packed, start = synth.pack_reads_for_build(reads)
    ost = oracle.Stream.build(packed, start, k, threads=4)
    oes = ost.edges()
    assert oes.large.size > 0                                             # the `large` path is exercised: counts above 254 exist
    og = oracle.Graph(ost)
    mult = oracle_mult(oes)
    stream = ctx.build_sdbg(ctx.upload_reads(packed, start), k)
    assert stream.md5() == oes.md5()
    g = api.Graph(ctx, stream, keep_multiplicity=True)
    strs = ["".join(DNA[c] for c in r) for r in reads]
    return dict(k=k, reads=reads, strs=strs, og=og, mult=mult, g=g, stream=stream, packed=packed, start=start)


# ---- 2. counts above 254: oracle expectation AND brute-force count ---------------------------------------------------------------
def test_counts_above_254_equal_oracle_and_brute_force(hot):
    k, strs, g = hot["k"], hot["strs"], hot["g"]
    brute = Counter()
    for s in strs:
        for t in (s, rc(s)):
            for p in range(len(t) - k):
                brute[t[p:p + k + 1]] += 1
    uniq = list(dict.fromkeys(strs))                                      # the repeat once: its windows are the same 70 every time
    seqs = uniq + [rc(s) for s in uniq]
    want = [expected_windows(hot["og"], hot["mult"], s, k)[0] for s in seqs]
    bf = [[min(65535, brute[s[p:p + k + 1]]) for p in range(len(s) - k)] for s in seqs]
    disagree = sum(a != b for w, b_ in zip(want, bf) for a, b in zip(w, b_))
    assert disagree == 0, f"oracle stream and brute-force count disagree on {disagree} windows"
    assert sum(v >= 300 for v in want[len(uniq) - 1]) == 70 and sum(v >= 300 for v in want[-1]) == 70      # the repeat, both strands
    res = g.contig_coverage(seqs, per_window=True)
    check_call(res, seqs, k, want)
    check_call(res, seqs, k, bf)
    assert res["stats"]["n_index_searches"] == len(seqs)                  # reads lie wholly in the graph: one search each, the rest walked
    assert res["stats"]["n_walked"] == res["stats"]["n_windows"] - len(seqs)


def test_host_stream_without_its_large_words_is_refused(ctx, hot):
    """mgta_sdbg_load is not given the large words: under the switch a stream with records of 255 fails loudly, never a graph without counts"""
    import ctypes as C
    from megagta_amd import api
    s = hot["stream"]
    recs, bi, tips = np.ascontiguousarray(s.records), np.ascontiguousarray(s.bucket_items, dtype=np.int64), np.ascontiguousarray(s.tips)
    assert ((recs >> 8) == 255).any()
    load = lambda out: ctx._L.mgta_sdbg_load(ctx.h, s.k, recs.ctypes.data, recs.size, bi.ctypes.data, tips.ctypes.data, tips.size, s.words_per_tip, C.byref(out))
    out = C.c_void_p()
    ctx.keep_multiplicity(True)
    try:
        assert load(out) == -4 and not out.value and b"mgta_sdbg_load_large" in ctx._L.mgta_last_error()
        large = np.ascontiguousarray(s.large[:-1])                        # and the wrong number of large words is an error too
        assert ctx._L.mgta_sdbg_load_large(ctx.h, s.k, recs.ctypes.data, recs.size, bi.ctypes.data, tips.ctypes.data, tips.size, s.words_per_tip,
                                           large.ctypes.data, large.size, C.byref(out)) == -1 and not out.value
    finally:
        ctx.keep_multiplicity(False)
    assert load(out) == 0                                                 # without the switch the same call loads the graph it always did
    ctx._L.mgta_sdbg_free(out)


def test_worker_keeps_the_counted_graph_between_requests(ctx, hot, tmp_path):
    """`megagta serve`: the first `coverage` request loads the graph files with their counts, the next one (another gene of the run) uses
    that graph; both write what a one-shot `megagta coverage` writes"""
    from megagta_amd import api
    prefix = str(tmp_path / "g")
    api.write_sdbg(prefix, hot["stream"], num_files=2)
    fas = []
    for i, part in enumerate((hot["strs"][:200], hot["strs"][-350:])):
        fas.append(str(tmp_path / f"c{i}.fa"))
        open(fas[-1], "w").write("".join(f">c{j} x\n{s}\n" for j, s in enumerate(part)))
    for i, fa in enumerate(fas):
        subprocess.run([BIN, "coverage", prefix, fa, str(tmp_path / f"one{i}")], check=True, capture_output=True, timeout=120)
    req = "".join(f"coverage\t{prefix}\t{fa}\t{tmp_path}/w{i}\n" for i, fa in enumerate(fas)) + "quit\n"
    r = subprocess.run([BIN, "serve"], input=req, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["DONE", "0", "DONE", "0"], r.stderr[-2000:]
    assert r.stderr.count("with multiplicities: still on the device") == 1 and r.stderr.count("load with multiplicities") == 2
    for i in range(2):
        for suffix in ("_coverage.txt", "_abundance.txt"):
            a, b = open(f"{tmp_path}/one{i}{suffix}").read(), open(f"{tmp_path}/w{i}{suffix}").read()
            assert a == b and len(a) > 0, (i, suffix)
    rows = cv.read_coverage(f"{tmp_path}/w1_coverage.txt")
    assert len(rows) == 350 and all(r["covered"] == r["windows"] == 70 for r in rows) and max(r["max"] for r in rows) >= 300


def test_resident_multi_pass_stream_keeps_its_large_words(ctx, hot):
    """a kept multi-pass stream accumulates the large words beside its records when the switch is on, and says so when it was off"""
    from megagta_amd import api
    rd = ctx.upload_reads(hot["packed"], hot["start"])
    want = hot["g"].edge_multiplicity(np.arange(hot["g"].size))           # (== the oracle's: test above / test 1's route)
    assert np.array_equal(want, hot["mult"])
    try:
        ctx.set_mem_limit(10 << 20)
        ctx.keep_stream(True)
        ctx.keep_multiplicity(True)
        st = ctx.build_sdbg(rd, hot["k"], collect=False).stats
        assert st["n_passes"] >= 2 and st["n_large"] > 0
        for inplace in ("0", "1"):
            if inplace == "1":
                st = ctx.build_sdbg(rd, hot["k"], collect=False).stats
            os.environ["MGTA_LOAD_INPLACE"] = inplace
            try:
                g = api.Graph(ctx, None, hot["k"])
            finally:
                os.environ.pop("MGTA_LOAD_INPLACE", None)
            assert np.array_equal(g.edge_multiplicity(np.arange(g.size)), hot["mult"]), inplace
            g.free()
        ctx.keep_multiplicity(False)
        ctx.build_sdbg(rd, hot["k"], collect=False)
        with pytest.raises(api.MegaGtaError, match=r"\(-4\)"):           # never silently a graph without counts
            api.Graph(ctx, None, hot["k"], keep_multiplicity=True)
    finally:
        ctx.keep_multiplicity(False)
        ctx.set_mem_limit(0)
        ctx.keep_stream(False)


# ---- 3. contigs that leave the graph ----------------------------------------------------------------------------------------------
def leaving_contigs(strs, k, seed=5):
    rng = np.random.default_rng(seed)
    pick = lambda: strs[int(rng.integers(0, len(strs)))]
    out = []
    for _ in range(40):                                                   # two read substrings joined by 5 random bases
        a, b = pick(), pick()
        i, j = int(rng.integers(0, 40)), int(rng.integers(0, 40))
        out.append(a[i:i + 55] + "".join(DNA[c] for c in rng.integers(0, 4, 5)) + b[j:j + 55])
    for _ in range(10):                                                   # an N in the middle, at the start, at the end
        s = pick()
        p = int(rng.integers(0, 100))
        out.append(s[:p] + "N" + s[p + 1:])
    out += ["N" + pick()[1:], pick()[:-1] + "n", pick()[:50] + "NN" + pick()[52:]]
    for _ in range(10):                                                   # lower-case runs
        s = pick()
        p = int(rng.integers(0, 60))
        out.append(s[:p] + s[p:p + 40].lower() + s[p + 40:])
    out += [pick().lower(), pick()[:k], pick()[:5], "", pick()[:k + 1], pick()[10:10 + k + 1], "ACGT" * 30]      # shorter than k + 1, exactly k + 1, foreign
    return out


def test_contigs_that_leave_the_graph(hot):
    k, g = hot["k"], hot["g"]
    seqs = leaving_contigs(hot["strs"], k)
    exp = [expected_windows(hot["og"], hot["mult"], s, k) for s in seqs]
    res = g.contig_coverage(seqs, per_window=True)
    check_call(res, seqs, k, [e[0] for e in exp])
    assert any(0 in e[0] and max(e[0]) > 0 for e in exp)                  # some contig really leaves the graph and comes back
    st = res["stats"]
    assert st["n_contigs"] == len(seqs) and st["n_walked"] + st["n_index_searches"] <= st["n_windows"]
    # an empty batch
    res0 = g.contig_coverage([], per_window=True)
    assert res0["contigs"].size == 0 and res0["per_window"].size == 0 and not res0["abundance"].any() and res0["stats"]["n_windows"] == 0
    # contigs that lie wholly in the graph need ONE index search each (a condition: it is what shows that the walk is used)
    inside = [s for s, e in zip(seqs, exp) if e[1] and min(e[1]) >= 0]
    inside += list(dict.fromkeys(hot["strs"]))[:200]
    r2 = g.contig_coverage(inside)
    assert len(inside) > 200 and r2["stats"]["n_index_searches"] == len(inside)
    assert r2["stats"]["n_walked"] == r2["stats"]["n_windows"] - len(inside)


# ---- 4. abundance -----------------------------------------------------------------------------------------------------------------
def test_abundance_counts_distinct_edges(hot):
    k, g, mult = hot["k"], hot["g"], hot["mult"]
    seqs = leaving_contigs(hot["strs"], k) + list(dict.fromkeys(hot["strs"]))[-300:]
    ids = np.array([e for s in seqs for e in expected_windows(hot["og"], mult, s, k)[1] if e >= 0], dtype=np.int64)
    want = np.bincount(mult[np.unique(ids)], minlength=65536)
    assert want[300:].sum() > 0                                           # bins above the ones a workgroup counts in LDS are used
    got = g.contig_coverage(seqs)["abundance"]
    assert np.array_equal(got, want)
    assert np.array_equal(g.contig_coverage(seqs + seqs[:50] + seqs[:50])["abundance"], want)      # the same contig three times changes nothing
    assert g.contig_coverage(seqs, abundance=False)["abundance"] is None


# ---- 5. off means off -------------------------------------------------------------------------------------------------------------
def test_off_means_off(ctx, oracle, golden_dir):
    from megagta_amd import api
    d = os.path.join(golden_dir, "toy")
    packed, start = readlib.load_for_build(os.path.join(d, "reads.lib"))
    stream = ctx.build_sdbg(ctx.upload_reads(packed, start), 44)
    g_off, g_on = api.Graph(ctx, stream), api.Graph(ctx, stream, keep_multiplicity=True)
    with pytest.raises(api.MegaGtaError, match=r"\(-1\)"):
        g_off.edge_multiplicity([0])
    with pytest.raises(api.MegaGtaError, match=r"\(-1\)"):
        g_off.contig_coverage(["A" * 60])
    fw = api.DeviceHmm(ctx, hmmlib.parse_hmm(os.path.join(d, "for_enone.hmm")))
    rv = api.DeviceHmm(ctx, hmmlib.parse_hmm(os.path.join(d, "rev_enone.hmm")))
    gold = H.parse_probe_astar(H.gz_lines(os.path.join(d, "astar_cold.txt.gz")))
    kmers, states = [r["kmer"] for r in gold], [r["start_state"] for r in gold]
    a, _ = api.astar_search(g_off, fw, rv, kmers, states, 20, 0.5)
    b, _ = api.astar_search(g_on, fw, rv, kmers, states, 20, 0.5)
    assert [(x.left, x.right, x.right_side, x.left_side) for x in a] == [(x.left, x.right, x.right_side, x.left_side) for x in b]
    assert [x.contig(km) for x, km in zip(a, kmers)] == [r["contig"] for r in gold]
    fa, sa = g_off.denovo(150, False, 46)
    fb, sb = g_on.denovo(150, False, 46)
    assert fa == fb and len(fa) > 0 and {n: v for n, v in sa.items() if not n.startswith("ms_")} == {n: v for n, v in sb.items() if not n.startswith("ms_")}
    # the counts survive what denovo did to the validity bits
    assert np.array_equal(g_on.edge_multiplicity(np.arange(g_on.size)), oracle_mult(oracle.Stream.build(packed, start, 44, threads=4).edges()))


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------------
def _tree(root):
    out = {}
    for dp, _, fs in os.walk(root):
        for f in fs:
            p = os.path.join(dp, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def test_driver_coverage_end_to_end(ctx, oracle, golden_dir, tmp_path):
    from megagta_amd import api
    assert os.path.exists(BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    mg = synth.make_metagenome(6000, 150, (("rplB", 100),), seed=11, reads_per_genome=1000)    # the sample of test_process_boundary_gpu.py
    synth.write_fasta(mg.reads, str(tmp_path / "reads.fa"))
    toy = os.path.join(golden_dir, "toy")
    (tmp_path / "gene_list.txt").write_text(f"rplB {toy}/for_enone.hmm {toy}/rev_enone.hmm {toy}/ref_aligned.faa\n")
    base = [sys.executable, DRIVER, "-r", str(tmp_path / "reads.fa"), "-g", str(tmp_path / "gene_list.txt"), "-k", "45", "-t", "4", "--min-contig-len", "150"]
    runs = {"plain": [], "cov": ["--coverage"], "cov_1p": ["--coverage", "--one-process-per-step"]}
    trees = {}
    for name, extra in runs.items():
        out = tmp_path / name
        r = subprocess.run(base + ["-o", str(out)] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr + open(out / "log").read()[-2000:]
        trees[name] = _tree(str(out))
    new = {"contigs/rplB/nucl_merged_coverage.txt", "contigs/rplB/nucl_merged_abundance.txt"}
    volatile = {"log", "opts.txt", "tmp/cp.txt"}                          # time stamps; the flag itself; the two extra checkpoints
    for name in ("cov", "cov_1p"):
        assert set(trees[name]) == set(trees["plain"]) | new
        for f, data in trees["plain"].items():                            # the FASTA and every other output file: byte-identical without the flag
            if f not in volatile:
                assert trees[name][f] == data, (name, f)
    for f in new:                                                         # both process models: identical files
        assert trees["cov"][f] == trees["cov_1p"][f] and len(trees["cov"][f]) > 0, f
    cp_plain = trees["plain"]["tmp/cp.txt"].decode().splitlines()
    cp_cov = trees["cov"]["tmp/cp.txt"].decode().splitlines()
    assert cp_cov[:len(cp_plain)] == cp_plain and len(cp_cov) == len(cp_plain) + 1 and cp_cov == trees["cov_1p"]["tmp/cp.txt"].decode().splitlines()
    # one row per record of nucl_merged.fasta, in order; every row == the API == the oracle
    out = tmp_path / "cov"
    names, seqs = cv.read_fasta(str(out / "contigs" / "rplB" / "nucl_merged.fasta"))
    rows = cv.read_coverage(str(out / "contigs" / "rplB" / "nucl_merged_coverage.txt"))
    assert [r["contig"] for r in rows] == names and len(names) > 10
    k = 44
    g = api.Graph.from_files(ctx, str(out / "k44" / "44"), keep_multiplicity=True)
    res = g.contig_coverage(seqs, per_window=True)
    assert cv.coverage_text(names, res["contigs"]).encode() == trees["cov"]["contigs/rplB/nucl_merged_coverage.txt"]
    assert cv.abundance_text(res["abundance"]).encode() == trees["cov"]["contigs/rplB/nucl_merged_abundance.txt"]
    ost = oracle.Stream.read(str(out / "k44" / "44"))
    og, mult = oracle.Graph(ost), oracle_mult(ost.edges())
    exp = [expected_windows(og, mult, s, k) for s in seqs]
    check_call(res, seqs, k, [e[0] for e in exp])
    all_ids = []
    for r, s, (w, ids) in zip(rows, seqs, exp):
        st = cv.stats_of_windows(w, len(s))
        assert all(r[c] == st[c] for c in ("len", "windows", "covered", "median", "min", "max")) and r["mean"] == float("%.4f" % (st["sum"] / st["windows"]))
        # the contigs of the search are paths of this very graph: every window has an edge, by the oracle's own index_edge
        assert r["covered"] == sum(e >= 0 for e in ids) == r["windows"], r["contig"]
        all_ids += [e for e in ids if e >= 0]
    assert np.array_equal(cv.read_abundance(str(out / "contigs" / "rplB" / "nucl_merged_abundance.txt")), np.bincount(mult[np.unique(all_ids)], minlength=65536))
    # --continue on a finished run with the flag does nothing and succeeds
    before = trees["cov"]["contigs/rplB/nucl_merged_coverage.txt"]
    r = subprocess.run([sys.executable, DRIVER, "--continue", "-o", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and open(out / "contigs" / "rplB" / "nucl_merged_coverage.txt", "rb").read() == before


# ---- 7. determinism ---------------------------------------------------------------------------------------------------------------
def test_two_runs_give_identical_bytes(hot):
    k, g = hot["k"], hot["g"]
    seqs = leaving_contigs(hot["strs"], k) + hot["strs"][:400]
    a, b = g.contig_coverage(seqs, per_window=True), g.contig_coverage(seqs, per_window=True)
    for key in ("contigs", "per_window", "abundance"):
        assert a[key].tobytes() == b[key].tobytes(), key
    assert {n: v for n, v in a["stats"].items() if not n.startswith("ms_")} == {n: v for n, v in b["stats"].items() if not n.startswith("ms_")}
    # and cutting the call into many batches changes nothing (the marks live across the batches of a call)
    g.ctx.set_coverage_batch(1000)
    try:
        c = g.contig_coverage(seqs, per_window=True)
    finally:
        g.ctx.set_coverage_batch(0)
    assert a["stats"]["n_batches"] == 1 and c["stats"]["n_batches"] > 5
    assert a["stats"]["groups_per_cu"] >= 32 and a["stats"]["groups_per_cu"] % 32 == 0
    for key in ("contigs", "per_window", "abundance"):
        assert a[key].tobytes() == c[key].tobytes(), key
