"""Read recruitment (Graph.match_reads / `megagta matchreads` / `megagta.py --match-reads`): the reads that share a (k+1)-mer with a
set of contigs, on either strand.

Expected values never come from the code under test.  On a `-m 1` graph of the reads themselves a hit is string equality of
(k+1)-mers, so the expectation is Python sets over strings; where strings are not enough (`-m 2 --need_mercy`: a read window need not
be an edge) it is the CPU oracle's IndexBinarySearchEdge.  Every comparison is exact: the outputs are integers and bits."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from megagta_amd import hmm as hmmlib
from megagta_amd import matchreads as mr
from megagta_amd import readlib, synth
from tests import helpers as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "megagta_amd", "bin", "megagta")
DRIVER = os.path.join(ROOT, "megagta_amd", "megagta.py")
DNA = "ACGT"
COMP = str.maketrans("ACGTacgt", "TGCAtgca")
K = 30
SHORT_LENS = (5, 30, 31, 32, 47, 48, 49)      # below k + 1, exactly k + 1, around the 16-base word boundaries


def rc(s):
    return s.translate(COMP)[::-1]


def to_str(codes):
    return "".join(DNA[c] for c in codes)


def windows(s, k):
    return [s[p:p + k + 1] for p in range(len(s) - k)]


def contig_window_set(contigs, k):
    """the ACGT-only windows of the contigs as given (upper-cased); no N -> G folding"""
    return {w for c in contigs for w in windows(c.upper(), k) if set(w) <= set(DNA)}


def brute_force_hits(strs, contigs, k):
    """hit_windows by string equality on either strand, and the number of marked edges: len(set(windows) | set(rc windows)) over the
    contig windows that ARE edges of the `-m 1` graph of `strs`, i.e. (k+1)-mers of a read on either strand -- a window without an
    edge (the foreign contig's, a stretch of the genome no read covers) marks nothing"""
    cw = contig_window_set(contigs, k)
    both = cw | {rc(w) for w in cw}
    edges = {w for s in strs for w in windows(s, k)}
    edges |= {rc(w) for w in edges}
    return np.array([sum(w in both for w in windows(s, k)) for s in strs], dtype=np.uint32), len(both & edges)


def no_ms(stats):
    return {n: v for n, v in stats.items() if not n.startswith("ms_")}


@pytest.fixture(scope="module")
def ctx():
    from megagta_amd import api
    c = api.Context(0)
    yield c
    c.close()


def make_library(seed=33):
    """1500 reads of 100 bp from a random 5 kb genome A (odd ones reverse-complemented), 500 from an unrelated genome B, and reads of
    SHORT_LENS from A; the contigs of test 1, built from the known read positions"""
    rng = np.random.default_rng(seed)
    A, B = rng.integers(0, 4, 5000).astype(np.uint8), rng.integers(0, 4, 5000).astype(np.uint8)
    sa = to_str(A)
    reads, pos_a = [], []
    for i in range(1500):
        p = int(rng.integers(0, 5000 - 100 + 1))
        r = A[p:p + 100]
        pos_a.append(p)
        reads.append(((3 - r)[::-1] if i % 2 else r).copy())
    for i in range(500):
        p = int(rng.integers(0, 5000 - 100 + 1))
        r = B[p:p + 100]
        reads.append(((3 - r)[::-1] if i % 2 else r).copy())
    short_at = len(reads)
    for j, n in enumerate(SHORT_LENS):
        reads.append(A[200 * j + 7:200 * j + 7 + n].copy())
    # the ten substrings, the N, lower-case and short contigs all lie in A[0:3500); the two one-window contigs lie beyond, around a
    # forward read each, far enough apart that neither touches the other's read
    contigs = []
    for _ in range(10):
        n = int(rng.integers(200, 401))
        p = int(rng.integers(0, 3500 - n))
        contigs.append(sa[p:p + n])
    with_n = sa[1000:1075] + "N" + sa[1076:1150]
    contigs += [with_n, sa[2000:2150].lower(), sa[100:100 + K], to_str(rng.integers(0, 4, 200))]
    first_r = next(i for i in range(0, 1500, 2) if 3700 <= pos_a[i] <= 4200)
    last_r = next(i for i in range(0, 1500, 2) if 4400 <= pos_a[i] <= 4800)
    p, q = pos_a[first_r], pos_a[last_r]
    contigs.append(sa[p + K + 1 - 40:p + K + 1])                          # ends with the first window of read first_r
    contigs.append(sa[q + 100 - K - 1:q + 100 - K - 1 + 40])              # starts with the last window of read last_r
    return dict(A=sa, reads=reads, contigs=contigs, n_a=1500, n_b=500, short_at=short_at, first_r=first_r, last_r=last_r)


@pytest.fixture(scope="module")
def lib(ctx):
    """the library of test 1 on the device, its `-m 1` graph loaded WITHOUT multiplicities, and the brute-force expectation"""
    from megagta_amd import api
    d = make_library()
    packed, start = readlib.pack_for_build(d["reads"])
    rd = ctx.upload_reads(packed, start)
    stream = ctx.build_sdbg(rd, K)
    g = api.Graph(ctx, stream)
    strs = [to_str(r) for r in d["reads"]]
    want, n_marked = brute_force_hits(strs, d["contigs"], K)
    n_all = len(contig_window_set(d["contigs"], K) | {rc(w) for w in contig_window_set(d["contigs"], K)})
    assert 0 < n_marked < n_all                                          # some contig windows have no edge (the foreign contig's)
    d.update(packed=packed, start=start, rd=rd, stream=stream, g=g, strs=strs, want=want, n_marked=n_marked,
             n_windows=np.array([max(0, len(s) - K) for s in strs], dtype=np.int64))
    return d


# ---- 1. brute force, both strands, -m 1 -------------------------------------------------------------------------------------------
def test_brute_force_both_strands(lib):
    want, nw, n_a, n_b, short_at = lib["want"], lib["n_windows"], lib["n_a"], lib["n_b"], lib["short_at"]
    # the inputs are not vacuous
    assert (want[:n_a] > 0).any() and (want[:n_a] == 0).any()
    assert (want[1:n_a:2] > 0).any()                                      # reverse-complemented reads are among the matches
    assert not want[n_a:n_a + n_b].any()                                  # no read of the unrelated genome
    both = contig_window_set(lib["contigs"], K)
    both |= {rc(w) for w in both}
    for r, at in ((lib["first_r"], 0), (lib["last_r"], 100 - K - 1)):     # one window only: the read's first / last
        assert want[r] == 1 and windows(lib["strs"][r], K)[at] in both, (r, at)
    assert [len(s) for s in lib["strs"][short_at:]] == list(SHORT_LENS)
    assert nw[short_at:].tolist() == [0, 0, 1, 2, 17, 18, 19] and not want[short_at:short_at + 2].any()
    assert any("N" in c for c in lib["contigs"]) and any(c.islower() for c in lib["contigs"]) and any(len(c) == K for c in lib["contigs"])
    g, rd = lib["g"], lib["rd"]
    full = g.match_reads(rd, lib["contigs"], counts=True)
    fast = g.match_reads(rd, lib["contigs"])
    assert full["hit_windows"].dtype == np.uint32 and np.array_equal(full["hit_windows"], want)
    assert fast["hit_windows"] is None
    for res in (full, fast):
        assert res["bits"].dtype == bool and np.array_equal(res["bits"], want > 0)
        st = res["stats"]
        assert st["n_matched_reads"] == int((want > 0).sum()) and st["n_reads"] == len(want)
        assert st["n_read_windows"] == int(nw.sum())
        assert st["n_contigs"] == len(lib["contigs"]) and st["n_contig_windows"] == sum(max(0, len(c) - K) for c in lib["contigs"])
        assert st["n_marked_edges"] == lib["n_marked"]
        assert st["groups_per_cu"] >= 32 and st["groups_per_cu"] % 32 == 0


# ---- 2. the walk is used, and the early exit is real ------------------------------------------------------------------------------
def test_walk_is_used_and_early_exit_is_real(lib):
    g, rd, nw, n_a, n_b = lib["g"], lib["rd"], lib["n_windows"], lib["n_a"], lib["n_b"]
    st = g.match_reads(rd, lib["contigs"], counts=True)["stats"]
    assert st["n_index_searches"] == int((nw > 0).sum())                  # every read lies wholly in its own -m 1 graph: one search each
    assert st["n_walked"] == st["n_read_windows"] - st["n_index_searches"]
    # the whole genome as the contig: every read of A hits at its first window and is walked no further
    res = g.match_reads(rd, [lib["A"]])
    is_a = np.ones(len(nw), dtype=bool)
    is_a[n_a:n_a + n_b] = False
    assert np.array_equal(res["bits"], is_a & (nw > 0))
    assert res["stats"]["n_walked"] == int((nw[n_a:n_a + n_b] - 1).sum())
    assert res["stats"]["n_index_searches"] == int((nw > 0).sum())
    full = g.match_reads(rd, [lib["A"]], counts=True)
    assert np.array_equal(full["hit_windows"], np.where(is_a, nw, 0))     # and with counts every window of those reads hits
    assert full["stats"]["n_walked"] == int((nw[nw > 0] - 1).sum())


# ---- 3. against the oracle's graph where strings are not enough -------------------------------------------------------------------
@pytest.mark.parametrize("case", ["toy_m2_mercy", "ragged"])
def test_against_the_oracle_graph(ctx, oracle, golden_dir, case):
    from megagta_amd import api
    name, k, m, mercy = ("toy", 44, 2, True) if case == "toy_m2_mercy" else ("ragged", 29, 1, False)
    codes = readlib.load_lib_bin(os.path.join(golden_dir, name, "reads.lib"))
    packed, start = readlib.pack_for_build(codes)
    ost = oracle.Stream.build_solid(packed, start, k, m, mercy, threads=4) if m > 1 else oracle.Stream.build(packed, start, k, threads=4)
    og = oracle.Graph(ost)
    rd = ctx.upload_reads(packed, start)
    stream = ctx.build_sdbg(rd, k, min_count=m, need_mercy=mercy)
    assert stream.md5() == ost.edges().md5()
    g = api.Graph(ctx, stream)
    # the graph is the whole library's; the scan takes its first reads (n_short_reads), which keeps the oracle's one-call-per-window
    # expectation within seconds on the 6000-read library
    n_scan = min(len(codes), 1500)
    strs = [to_str(c) for c in codes[:n_scan]]
    cache = {}

    def edge(w):
        e = cache.get(w)
        if e is None:
            e = cache[w] = og.index_edge(w)
        return e

    pick = [s for s in strs if len(s) >= 120][:: max(1, len(strs) // 12)][:12]
    assert len(pick) >= 6
    contigs = [s[10:110] for s in pick[:8]] + pick[8:]
    marked = {edge(w) for c in contigs for w in windows(c, k)} | {edge(rc(w)) for c in contigs for w in windows(c, k)}
    marked.discard(-1)
    ids = [[edge(w) for w in windows(s, k)] for s in strs]
    want = np.array([sum(e in marked for e in row) for row in ids], dtype=np.uint32)
    assert (want > 0).any() and (want == 0).any()
    full, fast = g.match_reads(rd, contigs, n_short_reads=n_scan, counts=True), g.match_reads(rd, contigs, n_short_reads=n_scan)
    assert np.array_equal(full["hit_windows"], want)
    assert np.array_equal(full["bits"], want > 0) and np.array_equal(fast["bits"], want > 0)
    assert full["stats"]["n_marked_edges"] == len(marked) and fast["stats"]["n_matched_reads"] == int((want > 0).sum())
    if m > 1:
        # the restart path: a read leaves the graph (a window without an edge) and comes back (windows with edges behind it)
        assert any(-1 in row and max(row[row.index(-1):]) >= 0 for row in ids)
        assert full["stats"]["n_index_searches"] > len(strs)
    else:
        assert full["stats"]["n_index_searches"] == sum(len(s) > k for s in strs)
    g.free()


# ---- 4. independence from the rest ------------------------------------------------------------------------------------------------
def test_independent_of_multiplicities_and_coverage(ctx, lib):
    from megagta_amd import api
    g, rd, want = lib["g"], lib["rd"], lib["want"]
    with pytest.raises(api.MegaGtaError, match=r"\(-1\)"):               # a graph loaded without the switch still has no counts
        g.contig_coverage(lib["contigs"])
    g_on = api.Graph(ctx, lib["stream"], keep_multiplicity=True)
    cov_seqs = lib["strs"][:300]
    before = g_on.contig_coverage(cov_seqs)["abundance"].tobytes()
    a = g_on.match_reads(rd, lib["contigs"], counts=True)
    assert g_on.contig_coverage(cov_seqs)["abundance"].tobytes() == before
    b = g_on.match_reads(rd, lib["contigs"], counts=True)
    assert np.array_equal(a["hit_windows"], want)
    assert a["hit_windows"].tobytes() == b["hit_windows"].tobytes() and a["bits"].tobytes() == b["bits"].tobytes()
    assert no_ms(a["stats"]) == no_ms(b["stats"])
    g_on.free()


def test_empty_inputs_and_a_prefix_of_the_library(lib):
    g, rd, want, nw = lib["g"], lib["rd"], lib["want"], lib["n_windows"]
    res = g.match_reads(rd, [], counts=True)
    assert res["bits"].size == len(want) and not res["bits"].any() and not res["hit_windows"].any()
    assert all(v == 0 for v in res["stats"].values())
    res = g.match_reads(rd, lib["contigs"], n_short_reads=0, counts=True)
    assert res["bits"].size == 0 and res["hit_windows"].size == 0 and all(v == 0 for v in res["stats"].values())
    half = len(want) // 2
    res = g.match_reads(rd, lib["contigs"], n_short_reads=half, counts=True)
    assert res["bits"].size == half and np.array_equal(res["hit_windows"], want[:half]) and np.array_equal(res["bits"], want[:half] > 0)
    assert res["stats"]["n_reads"] == half and res["stats"]["n_read_windows"] == int(nw[:half].sum())
    assert res["stats"]["n_matched_reads"] == int((want[:half] > 0).sum())


def test_search_is_untouched_by_the_marks(ctx, golden_dir):
    from megagta_amd import api
    d = os.path.join(golden_dir, "toy")
    codes = readlib.load_lib_bin(os.path.join(d, "reads.lib"))
    packed, start = readlib.pack_for_build(codes)
    rd = ctx.upload_reads(packed, start)
    g = api.Graph(ctx, ctx.build_sdbg(rd, 44))
    res = g.match_reads(rd, [to_str(c) for c in codes[:40]])
    assert res["bits"][:40].all() and res["stats"]["n_marked_edges"] > 0
    fw = api.DeviceHmm(ctx, hmmlib.parse_hmm(os.path.join(d, "for_enone.hmm")))
    rv = api.DeviceHmm(ctx, hmmlib.parse_hmm(os.path.join(d, "rev_enone.hmm")))
    gold = H.parse_probe_astar(H.gz_lines(os.path.join(d, "astar_cold.txt.gz")))
    kmers, states = [r["kmer"] for r in gold], [r["start_state"] for r in gold]
    got, _ = api.astar_search(g, fw, rv, kmers, states, 20, 0.5)
    assert [x.contig(km) for x, km in zip(got, kmers)] == [r["contig"] for r in gold]
    g.free()


# ---- 5. determinism ---------------------------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bytes(lib):
    g, rd = lib["g"], lib["rd"]
    for counts in (True, False):
        a, b = g.match_reads(rd, lib["contigs"], counts=counts), g.match_reads(rd, lib["contigs"], counts=counts)
        assert a["bits"].tobytes() == b["bits"].tobytes() and no_ms(a["stats"]) == no_ms(b["stats"])
        if counts:
            assert a["hit_windows"].tobytes() == b["hit_windows"].tobytes()


# ---- 6. guards --------------------------------------------------------------------------------------------------------------------
def test_guards(lib):
    from megagta_amd import api
    g, rd = lib["g"], lib["rd"]
    L = g.ctx._L
    off = np.array([0, 40], dtype=np.uint64)
    st = g.match_reads(rd, ["A" * 40])["stats"]                           # (the same arguments with a buffer are a valid call)
    assert st["n_contigs"] == 1
    assert L.mgta_reads_match_contigs(g.h, rd.h, 1, rd.n_reads, b"A" * 40, off.ctypes.data, 1, None, None, None) == -1
    assert b"match_bits" in L.mgta_last_error()
    words = np.zeros(rd.n_reads // 64 + 2, dtype=np.uint64)
    assert L.mgta_reads_match_contigs(None, rd.h, 1, rd.n_reads, b"A" * 40, off.ctypes.data, 1, words.ctypes.data, None, None) == -1
    assert L.mgta_reads_match_contigs(g.h, None, 1, rd.n_reads, b"A" * 40, off.ctypes.data, 1, words.ctypes.data, None, None) == -1
    with pytest.raises(api.MegaGtaError, match=r"\(-1\).*n_short_reads"):
        g.match_reads(rd, ["A" * 40], n_short_reads=rd.n_reads + 1)
    other = api.Context(0)
    try:
        rd2 = other.upload_reads(lib["packed"], lib["start"])
        with pytest.raises(api.MegaGtaError, match=r"\(-1\).*different contexts"):
            g.match_reads(rd2, ["A" * 40])
        rd2.free()
    finally:
        other.close()
    assert not words.any()                                                # nothing was written by the refused calls


# ---- 7. process boundary ----------------------------------------------------------------------------------------------------------
def write_ragged_lib(reads, prefix):
    """reads.lib.bin / .lib_info of reads of any lengths: per read uint32 length + ceil(length / 16) words, forward orientation"""
    parts = []
    for r in reads:
        parts += [np.array([r.size], dtype=np.uint32), readlib.pack_codes(r)]
    np.concatenate(parts).tofile(prefix + ".bin")
    with open(prefix + ".lib_info", "w") as f:
        f.write(f"{sum(r.size for r in reads)} {len(reads)}\nsynthetic.fa\n0 {len(reads) - 1} {max(r.size for r in reads)} se\n")


def test_one_shot_and_worker_write_the_same_file(lib, tmp_path):
    from megagta_amd import api
    assert os.path.exists(BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    prefix, libp = str(tmp_path / "g"), str(tmp_path / "reads.lib")
    api.write_sdbg(prefix, lib["stream"], num_files=2)
    write_ragged_lib(lib["reads"], libp)
    sets = (lib["contigs"], [lib["A"][4000:4400], "ACGT" * 20])
    fas = []
    for i, contigs in enumerate(sets):
        fas.append(str(tmp_path / f"c{i}.fa"))
        open(fas[-1], "w").write("".join(f">c{j} x\n{s}\n" for j, s in enumerate(contigs)))
    for i, fa in enumerate(fas):
        subprocess.run([BIN, "matchreads", prefix, libp, fa, str(tmp_path / f"one{i}")], check=True, capture_output=True, timeout=120)
    req = "".join(f"matchreads\t{prefix}\t{libp}\t{fa}\t{tmp_path}/w{i}\n" for i, fa in enumerate(fas)) + "quit\n"
    r = subprocess.run([BIN, "serve"], input=req, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["DONE", "0", "DONE", "0"], r.stderr[-2000:]
    assert r.stderr.count(f"graph {prefix}: still on the device") == 1 and r.stderr.count("library: still in memory") == 1
    for i, contigs in enumerate(sets):
        one, w = open(f"{tmp_path}/one{i}_match_reads.fa").read(), open(f"{tmp_path}/w{i}_match_reads.fa").read()
        bits = lib["g"].match_reads(lib["rd"], contigs)["bits"]
        assert one == w == mr.match_reads_text(bits, lib["packed"], lib["start"]) and len(one) > 0, i
        idx, seqs = mr.parse_match_reads(one)
        assert idx.tolist() == np.flatnonzero(bits).tolist() and seqs == [lib["strs"][j] for j in idx]


# ---- 8. driver end to end ---------------------------------------------------------------------------------------------------------
def _tree(root):
    out = {}
    for dp, _, fs in os.walk(root):
        for f in fs:
            p = os.path.join(dp, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def test_driver_match_reads_end_to_end(golden_dir, tmp_path):
    assert os.path.exists(BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    mg = synth.make_metagenome(6000, 150, (("rplB", 100),), seed=11, reads_per_genome=1000)    # the sample of the coverage test
    synth.write_fasta(mg.reads, str(tmp_path / "reads.fa"))
    toy = os.path.join(golden_dir, "toy")
    (tmp_path / "gene_list.txt").write_text(f"rplB {toy}/for_enone.hmm {toy}/rev_enone.hmm {toy}/ref_aligned.faa\n")
    base = [sys.executable, DRIVER, "-r", str(tmp_path / "reads.fa"), "-g", str(tmp_path / "gene_list.txt"), "-k", "45", "-t", "4", "--min-contig-len", "150"]
    runs = {"mr": ["--match-reads"], "cov_mr_1p": ["--coverage", "--match-reads", "--one-process-per-step"]}
    trees = {}
    for name, extra in runs.items():
        out = tmp_path / name
        r = subprocess.run(base + ["-o", str(out)] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr + open(out / "log").read()[-2000:]
        trees[name] = _tree(str(out))
    new = "contigs/rplB/nucl_merged_match_reads.fa"
    assert trees["mr"][new] == trees["cov_mr_1p"][new] and len(trees["mr"][new]) > 0
    volatile = {"log", "opts.txt", "tmp/cp.txt"}
    shared = set(trees["mr"]) & set(trees["cov_mr_1p"])
    assert set(trees["cov_mr_1p"]) - set(trees["mr"]) == {"contigs/rplB/nucl_merged_coverage.txt", "contigs/rplB/nucl_merged_abundance.txt"}
    assert set(trees["mr"]) <= set(trees["cov_mr_1p"])
    for f in shared - volatile:
        assert trees["mr"][f] == trees["cov_mr_1p"][f], f
    # by brute force over the sample: exactly the reads that share a 45-mer with the gene's contigs, on either strand
    k = 44
    out = tmp_path / "mr"
    contigs = H.fasta_seqs(out / "contigs" / "rplB" / "nucl_merged.fasta")
    strs = [to_str(r) for r in mg.reads]
    want, _ = brute_force_hits(strs, contigs, k)
    idx, seqs = mr.parse_match_reads(trees["mr"][new].decode())
    assert idx.tolist() == np.flatnonzero(want > 0).tolist() and 0 < len(idx) < len(strs)
    assert seqs == [strs[i] for i in idx]
    # one checkpoint for the flag's step, behind every checkpoint of the steps before it (and behind --coverage's).  One k, one gene:
    # buildlib, buildgraph, findstart, then filterbylen + translate inside the search step and the search's own = 6 before the flag's
    cp_mr = trees["mr"]["tmp/cp.txt"].decode().splitlines()
    cp_both = trees["cov_mr_1p"]["tmp/cp.txt"].decode().splitlines()
    assert cp_mr == [f"{i}\tdone" for i in range(6 + 1)]
    assert cp_both[:len(cp_mr)] == cp_mr and len(cp_both) == len(cp_mr) + 1
    # --continue on the finished run does nothing and succeeds
    r = subprocess.run([sys.executable, DRIVER, "--continue", "-o", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and open(out / new, "rb").read() == trees["mr"][new]
