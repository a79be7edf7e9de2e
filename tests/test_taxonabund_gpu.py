"""Window-shared coverage (mgta_contig_share_coverage), `megagta sharecov` and `megagta.py --taxon-abund` on the device.

Expected values never come from the code under test.  Per window the edge id is oracle.Graph.index_edge of its k + 1 letters (none when
it holds a letter other than A, C, G, T), the multiplicity comes from the oracle's stream (records >> 8, the large words where that is
255), the shares are a collections.Counter over the edge ids of the call, and the masses are Python integers:
    mass(window) = (mult << 16) // share.
On the reads-only `-m 1` graph there is a second witness that does not go through the oracle's graph: a (k+1)-mer has an edge iff it
occurs in a read on either strand, and its share is the number of windows of the call equal to it, counted in numpy."""
import ctypes as C
import os
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

from megagta_amd import chimera as chimlib
from megagta_amd import cluster as clustlib
from megagta_amd import coverage as cv
from megagta_amd import nearest as nearlib
from megagta_amd import readlib, synth
from megagta_amd import taxonabund as ta

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "megagta_amd", "bin", "megagta")
DRIVER = os.path.join(ROOT, "megagta_amd", "megagta.py")
DNA = "ACGT"
COMP = str.maketrans("ACGTacgt", "TGCAtgca")
FIELDS = ("mass", "len", "n_windows", "n_covered", "n_unique", "max_share")


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
    assert int(big.sum()) == es.large.size
    m[big] = es.large
    return m


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
    return [np.asarray(r, dtype=np.uint8) for r in reads]


def contig_set(strs, k, seed):
    """about 40 contigs from reads (the LAST read is the one whose windows are to carry shares 3, 4 and 7): see the comments"""
    rng = np.random.default_rng(seed)
    a = strs[-1]
    long_reads = [s for s in dict.fromkeys(strs[:-1]) if len(s) >= k + 40 and s != a]
    pick = lambda: long_reads[int(rng.integers(0, len(long_reads)))]
    assert len(a) >= k + 55
    out = [a, pick(), a, pick(), a]                                       # one contig three times, not side by side
    out += [a[5:k + 50], a[20:k + 40], a[20:k + 40], a[20:k + 40]]        # pieces of it: shares 3 + 1 + 3 = 7 inside, 4 around, 3 outside
    b = pick()
    out += [b, b[3:k + 30]]                                               # a contig and a piece of it
    x = pick()[:k + 12]
    out += [x + x, x[:k + 5] + x[:k + 5] + x[:k + 5]]                     # internal repeats longer than k + 1: one edge twice / three times in ONE contig
    for _ in range(3):                                                    # an N; lower-case letters
        s = pick()
        p = int(rng.integers(k // 2, len(s) - k // 2))
        out.append(s[:p] + "N" + s[p + 1:])
    s = pick()
    out += [s[:10] + s[10:k + 20].lower() + s[k + 20:], pick().lower(), "n" + pick()[1:]]
    for _ in range(4):                                                    # leaves the graph and comes back
        s, t = pick(), pick()
        out.append(s[:k + 15] + "".join(DNA[c] for c in rng.integers(0, 4, 5)) + t[2:k + 17])
    s = pick()
    out += [s[:k], s[:k + 1], "", s[7:7 + k + 1], "ACGT" * 20]            # k, k + 1 and 0 letters; foreign
    out += [rc(pick()) for _ in range(3)] + [rc(a)]                       # the other strand: other edges
    while len(out) < 41:
        out.append(pick())
    return out


def windows_of(og, mult, seq, k):
    """-> (edge id per window or -1, multiplicity per window) from the oracle"""
    ids, ms = [], []
    for p in range(len(seq) - k):
        w = seq[p:p + k + 1].upper()
        e = og.index_edge(w) if set(w) <= set(DNA) else -1                # no N -> G folding
        ids.append(e)
        ms.append(int(mult[e]) if e >= 0 else 0)
    return ids, ms


def restate(og, mult, seqs, k):
    """the whole result of contig_share_coverage(seqs, per_window=True) in Python integers"""
    wins = [windows_of(og, mult, s, k) for s in seqs]
    share = Counter(e for ids, _ in wins for e in ids if e >= 0)
    rows, pws, pwm = [], [], []
    for s, (ids, ms) in zip(seqs, wins):
        sh = [share[e] if e >= 0 else 0 for e in ids]
        cov = [(m, c) for m, c in zip(ms, sh) if m > 0]
        rows.append(dict(mass=sum((m << 16) // c for m, c in cov), len=len(s), n_windows=len(ids), n_covered=len(cov), n_unique=sum(c == 1 for _, c in cov),
                         max_share=max((c for _, c in cov), default=0)))
        pws += sh
        pwm += ms
    return dict(rows=rows, per_window_share=pws, per_window=pwm, n_distinct_edges=len(share), total_mult=sum(int(mult[e]) for e in share),
                total_mass=sum(r["mass"] for r in rows), n_covered=sum(r["n_covered"] for r in rows), ids=wins)


def check_result(res, want):
    got = [{f: int(c[f]) for f in FIELDS} for c in res["contigs"]]
    for i, (g, w) in enumerate(zip(got, want["rows"])):
        assert g == w, (i, g, w)
    assert len(got) == len(want["rows"])
    assert res["per_window_share"].tolist() == want["per_window_share"]
    assert res["per_window"].tolist() == want["per_window"]
    st = res["stats"]
    for f in ("n_distinct_edges", "total_mult", "total_mass", "n_covered"):
        assert st[f] == want[f], (f, st[f], want[f])
    assert st["n_contigs"] == len(got) and st["n_windows"] == len(want["per_window"]) == int(res["window_offsets"][-1])


def stable(stats):
    return {n: v for n, v in stats.items() if not n.startswith("ms_") and n != "n_batches"}


@pytest.fixture(scope="module")
def cases(ctx, oracle, golden_dir):
    """the three graphs, each with its oracle, its contig set and the restatement of the call over it (computed once, never changed)"""
    from megagta_amd import api
    out = {}
    for name, k in (("toy", 44), ("ragged", 29), ("hot", 30)):
        reads = hot_reads() if name == "hot" else readlib.load_lib_bin(os.path.join(golden_dir, name, "reads.lib"))
        packed, start = readlib.pack_for_build(reads)
        ost = oracle.Stream.build(packed, start, k, threads=4)
        oes = ost.edges()
        og, mult = oracle.Graph(ost), oracle_mult(oes)
        stream = ctx.build_sdbg(ctx.upload_reads(packed, start), k)
        assert stream.md5() == oes.md5()
        g = api.Graph(ctx, stream, keep_multiplicity=True)
        strs = ["".join(DNA[c] for c in r) for r in reads]
        if name != "hot":                                                 # the read of the pieces: a long one
            strs.append(next(s for s in strs if len(s) >= k + 55))
        seqs = contig_set(strs, k, seed=len(name))
        out[name] = dict(k=k, g=g, og=og, mult=mult, strs=strs, seqs=seqs, want=restate(og, mult, seqs, k), stream=stream)
    assert out["hot"]["mult"].max() >= 300                                # a multiplicity above 254: the large words
    return out


# ---- 1. every field against the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["toy", "ragged", "hot"])
def test_every_field_equals_the_restatement(cases, name):
    c = cases[name]
    want, seqs, k = c["want"], c["seqs"], c["k"]
    # the set holds what it was made to hold
    sh, ms = want["per_window_share"], want["per_window"]
    assert max(sh) >= 7 and 0 in sh and any(-1 in ids and ids[0] >= 0 and ids[-1] >= 0 for ids, _ in want["ids"])      # ... leaves the graph and comes back
    for ids, _ in want["ids"][11:13]:                                     # one edge twice / three times in one contig
        found = [e for e in ids if e >= 0]
        assert len(found) - len(set(found)) >= 5
    assert {r["n_windows"] for r in want["rows"]} >= {0, 1} and {len(s) for s in seqs} >= {0, k, k + 1}
    assert any((m << 16) % s for m, s in zip(ms, sh) if s)                # the floor bites somewhere
    if name == "hot":                                                     # (nothing else of the set lies on the repeated read)
        assert {3, 4, 7} <= set(sh)
        assert any(m >= 300 and s == 3 for m, s in zip(ms, sh)) and any(m >= 300 and s == 7 and (m << 16) % 7 for m, s in zip(ms, sh))
    res = c["g"].contig_share_coverage(seqs, per_window=True)
    check_result(res, want)
    # n = 0
    r0 = c["g"].contig_share_coverage([], per_window=True)
    assert r0["contigs"].size == 0 and r0["per_window_share"].size == 0 and r0["per_window"].size == 0
    assert all(v == 0 for v in r0["stats"].values())
    # without the per-window outputs: the same records
    r1 = c["g"].contig_share_coverage(seqs)
    assert r1["per_window_share"] is None and r1["per_window"] is None and r1["contigs"].tobytes() == res["contigs"].tobytes()


def test_shares_equal_a_count_of_equal_windows(cases):
    """the second witness, on the reads-only -m 1 graph: no oracle graph, no edge ids"""
    c = cases["hot"]
    k, seqs = c["k"], c["seqs"]
    in_reads = set()
    for s in dict.fromkeys(c["strs"]):
        for t in (s, rc(s)):
            in_reads.update(t[p:p + k + 1] for p in range(len(t) - k))
    wins = [s[p:p + k + 1].upper() for s in seqs for p in range(len(s) - k)]
    uniq, inv, cnt = np.unique(np.array(wins), return_inverse=True, return_counts=True)
    has_edge = np.array([w in in_reads for w in uniq])                    # (a window with an N is in no read)
    want = np.where(has_edge[inv], cnt[inv], 0)
    res = c["g"].contig_share_coverage(seqs, per_window=True)
    assert np.array_equal(res["per_window_share"], want) and want.max() == 7
    assert res["stats"]["n_distinct_edges"] == int(has_edge.sum())


# ---- 2. the invariant; the walk is done once ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["toy", "ragged", "hot"])
def test_mass_invariant_and_one_walk(cases, name):
    c = cases[name]
    res = c["g"].contig_share_coverage(c["seqs"])
    st = res["stats"]
    mass = sum(int(m) for m in res["contigs"]["mass"])
    covered = sum(int(m) for m in res["contigs"]["n_covered"])
    print(f"{name}: total_mult {st['total_mult']}, sum of masses {mass}, covered windows {covered}, distinct edges {st['n_distinct_edges']}")
    assert mass == st["total_mass"] and covered == st["n_covered"]
    assert 65536 * st["total_mult"] - covered <= mass <= 65536 * st["total_mult"]
    assert st["total_mult"] == c["want"]["total_mult"]                    # (the bound is about the oracle's number, not the library's own)
    cov = c["g"].contig_coverage(c["seqs"])["stats"]
    assert st["n_walked"] == cov["n_walked"] and st["n_index_searches"] == cov["n_index_searches"] and st["n_windows"] == cov["n_windows"]
    assert st["table_bytes"] == 16 * st["table_slots"] and st["window_bytes"] == 4 * st["n_windows"]


# ---- 3. batches and collisions move nothing -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["toy", "hot"])
def test_batches_and_collisions_move_no_output(cases, name):
    c = cases[name]
    g, seqs = c["g"], c["seqs"]
    a = g.contig_share_coverage(seqs, per_window=True)
    runs = {}
    for what, batch, bits in (("batch", 64, 64), ("bits", 0, 2), ("both", 64, 1)):
        g.ctx.set_coverage_batch(batch)
        g.ctx.set_share_hash_bits(bits)
        try:
            runs[what] = g.contig_share_coverage(seqs, per_window=True)
        finally:
            g.ctx.set_coverage_batch(0)
            g.ctx.set_share_hash_bits(64)
    assert a["stats"]["n_batches"] == 1 and runs["batch"]["stats"]["n_batches"] > 5 and runs["bits"]["stats"]["n_batches"] == 1
    for what, b in runs.items():
        for key in ("contigs", "per_window_share", "per_window"):
            assert a[key].tobytes() == b[key].tobytes(), (what, key)
        assert stable(a["stats"]) == stable(b["stats"]), what
    check_result(runs["both"], c["want"])
    from megagta_amd import api
    for bad in (0, 65):
        with pytest.raises(api.MegaGtaError, match=r"\(-1\)"):
            g.ctx.set_share_hash_bits(bad)


# ---- 4. order and repetition --------------------------------------------------------------------------------------------------------
def test_reversed_order_and_twice(cases):
    c = cases["hot"]
    g, seqs = c["g"], c["seqs"]
    a, b, r = (g.contig_share_coverage(s, per_window=True) for s in (seqs, seqs, seqs[::-1]))
    for key in ("contigs", "per_window_share", "per_window"):
        assert a[key].tobytes() == b[key].tobytes(), key
    assert stable(a["stats"]) == stable(b["stats"]) == stable(r["stats"])
    assert a["contigs"][::-1].tobytes() == r["contigs"].tobytes()
    off = a["window_offsets"]
    back = np.concatenate([a["per_window_share"][off[i]:off[i + 1]] for i in range(len(seqs) - 1, -1, -1)])
    assert np.array_equal(back, r["per_window_share"])


# ---- 5. errors ----------------------------------------------------------------------------------------------------------------------
def test_graph_without_multiplicities_and_limits(ctx, cases):
    from megagta_amd import api
    c = cases["toy"]
    g_off = api.Graph(ctx, c["stream"])
    with pytest.raises(api.MegaGtaError, match=r"\(-1\).*mgta_ctx_keep_multiplicity"):
        g_off.contig_share_coverage(["A" * 60])
    g_off.free()
    # 2^32 windows or more: refused by name before anything is read or written (the letters are never touched)
    g = c["g"]
    big = 0xFFFFFFF0
    offsets = np.array([0, big, 2 * big], dtype=np.uint64)
    rec = np.full(2 * 32, 0xAB, dtype=np.uint8)
    st = api._lib.ShareStats()
    rc_ = ctx._L.mgta_contig_share_coverage(g.h, b"A", offsets.ctypes.data, 2, rec.ctypes.data, None, None, C.byref(st))
    assert rc_ == -1 and b"2^32" in ctx._L.mgta_last_error() and (rec == 0xAB).all()
    assert ctx._L.mgta_contig_share_coverage(g.h, b"A", offsets.ctypes.data, 1 << 31, rec.ctypes.data, None, None, C.byref(st)) == -1
    assert b"2^31" in ctx._L.mgta_last_error() and (rec == 0xAB).all()


# ---- 6. the command and the worker --------------------------------------------------------------------------------------------------
def test_sharecov_command_writes_the_restatement(cases, tmp_path):
    from megagta_amd import api
    c = cases["hot"]
    prefix = str(tmp_path / "g")
    api.write_sdbg(prefix, c["stream"], num_files=2)
    names = [f"c{i}" for i in range(len(c["seqs"]))]
    fa = str(tmp_path / "contigs.fa")
    open(fa, "w").write("".join(f">{n} some words\n{s}\n" for n, s in zip(names, c["seqs"])))
    want = ta.sharecov_text(names, c["want"]["rows"])
    subprocess.run([BIN, "sharecov", prefix, fa, str(tmp_path / "one")], check=True, capture_output=True, timeout=120)
    assert open(tmp_path / "one_sharecov.txt").read() == want
    rows = ta.read_sharecov(str(tmp_path / "one_sharecov.txt"))
    assert [r["contig"] for r in rows] == names and [r["mass"] for r in rows] == [ta.q16_to_e4(r["mass"]) for r in c["want"]["rows"]]
    # as requests to the worker: the graph `coverage` loaded with its counts serves `sharecov`, and the other way round
    req = f"coverage\t{prefix}\t{fa}\t{tmp_path}/w\nsharecov\t{prefix}\t{fa}\t{tmp_path}/w\nsharecov\t{prefix}\t{fa}\t{tmp_path}/w2\nquit\n"
    r = subprocess.run([BIN, "serve"], input=req, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["DONE", "0"] * 3, r.stderr[-2000:]
    assert r.stderr.count("with multiplicities: still on the device") == 2 and r.stderr.count("load with multiplicities") == 3
    assert open(tmp_path / "w_sharecov.txt").read() == want == open(tmp_path / "w2_sharecov.txt").read()
    r = subprocess.run([BIN, "sharecov", prefix, fa], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Usage: megagta sharecov" in r.stderr


# ---- 7. and 8. the driver -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver_inputs(golden_dir, tmp_path_factory):
    d = tmp_path_factory.mktemp("taxon_driver")
    mg = synth.make_metagenome(6000, 150, (("rplB", 100),), seed=11, reads_per_genome=1000)    # the sample of the other driver tests
    synth.write_fasta(mg.reads, str(d / "reads.fa"))
    toy = os.path.join(golden_dir, "toy")
    ref = open(os.path.join(toy, "ref_aligned.faa")).read().split("\n")[1]
    (d / "refs.faa").write_text(f">rplB_consensus Bacteria; Toyota; rplB of the toy genome\n{ref}\n>rplB_backwards\n{ref[::-1]}\n")
    (d / "gene_list.txt").write_text(f"rplB {toy}/for_enone.hmm {toy}/rev_enone.hmm {d}/refs.faa\n")
    base = [sys.executable, DRIVER, "-r", str(d / "reads.fa"), "-g", str(d / "gene_list.txt"), "-k", "45", "-t", "4", "--min-contig-len", "150"]
    return d, base


def abund_files(out):
    return sorted(f for _, _, files in os.walk(out) for f in files if "sharecov" in f or "abund" in f)


def test_driver_taxon_abund_end_to_end(ctx, driver_inputs):
    from megagta_amd import api
    tmp, base = driver_inputs
    out = tmp / "all"
    r = subprocess.run(base + ["-o", str(out), "--derep", "--align", "--cluster", "--nearest", "--chimera", "--taxon-abund"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + open(out / "log").read()[-2000:]
    d = out / "contigs" / "rplB"
    assert abund_files(out) == ["nucl_merged_rmdup_sharecov.txt", "prot_merged_rmdup_otu_abund.txt", "prot_merged_rmdup_taxon_abund.txt"]
    assert open(out / "tmp" / "cp.txt").read().splitlines() == [f"{i}\tdone" for i in range(6 + 6)]
    log = open(out / "log").read()
    assert log.index("for chimeras") < log.index("Computing the shared k-mer coverage of the contigs of rplB") < log.index("Summing the abundance of the clusters of rplB")
    # the three files parse; the masses of both tables sum to the total of the coverage file
    share = ta.read_sharecov(str(d / "nucl_merged_rmdup_sharecov.txt"))
    otu = ta.read_otu(str(d / "prot_merged_rmdup_otu_abund.txt"))
    taxon = ta.read_taxon(str(d / "prot_merged_rmdup_taxon_abund.txt"))
    total = sum(r["mass"] for r in share)
    assert total > 0 and sum(r["mass"] for r in otu) == total == sum(r["mass"] for r in taxon)
    assert sum(r["contigs"] for r in otu) == len(share) == sum(r["contigs"] for r in taxon) > 1
    assert sum(r["ppm"] for r in otu) <= 1000000 and sum(r["ppm"] for r in taxon) <= 1000000
    # one line per record of the nucleotide file of the cluster step, equal to the API on the graph of the run
    names, seqs = cv.read_fasta(str(d / "nucl_merged_rmdup.fasta"))
    assert [r["contig"] for r in share] == names
    g = api.Graph.from_files(ctx, str(out / "k44" / "44"), keep_multiplicity=True)
    res = g.contig_share_coverage(seqs)
    g.free()
    assert ta.sharecov_text(names, res["contigs"]) == open(d / "nucl_merged_rmdup_sharecov.txt").read()
    assert all(r["covered"] == r["windows"] for r in share)               # the contigs of the search are paths of this very graph
    # the tables are the join of the files of the steps before, and name the references with their lineage
    clust = clustlib.read_clust(str(d / "prot_merged_rmdup_clust.txt"))
    near = nearlib.read_nearest(str(d / "prot_merged_rmdup_rep_seqs_nearest.txt"))
    chim = chimlib.read_chimera(str(d / "prot_merged_rmdup_rep_seqs_chimera.txt"))
    otu2, taxon2 = ta.join(share, clust, near, chim, ta.read_ref_headers(str(tmp / "refs.faa")))
    assert ta.otu_text(otu2) == open(d / "prot_merged_rmdup_otu_abund.txt").read() and ta.taxon_text(taxon2) == open(d / "prot_merged_rmdup_taxon_abund.txt").read()
    assert [(r["ref"], r["lineage"]) for r in taxon] == [("rplB_consensus", "Bacteria; Toyota; rplB of the toy genome"), ("rplB_backwards", "-"), ("#chimeric", "-"),
                                                         ("#unassigned", "-")]
    assert len([r for r in otu if r["cluster"] is not None]) == int((clust["status"] == 0).sum())
    assert all(r["chimera"] in ("clean", "chimeric", "unchecked") for r in otu if r["cluster"] is not None)
    # --continue on the finished run does nothing and succeeds
    before = open(d / "prot_merged_rmdup_otu_abund.txt").read()
    r = subprocess.run([sys.executable, DRIVER, "--continue", "-o", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and open(d / "prot_merged_rmdup_otu_abund.txt").read() == before


def test_driver_without_the_flag_is_what_it_was(driver_inputs):
    tmp, base = driver_inputs
    out = tmp / "plain"
    r = subprocess.run(base + ["-o", str(out), "--align", "--cluster"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + open(out / "log").read()[-2000:]
    assert abund_files(out) == [] and open(out / "tmp" / "cp.txt").read().splitlines() == [f"{i}\tdone" for i in range(6 + 2)]
    log = open(out / "log").read()
    assert "shared k-mer coverage" not in log and "Summing the abundance" not in log
    # with the flag and without --nearest / --chimera: the per-cluster table alone, `-` where those steps would have spoken
    out2 = tmp / "otu_only"
    r = subprocess.run(base + ["-o", str(out2), "--align", "--cluster", "--taxon-abund"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + open(out2 / "log").read()[-2000:]
    assert abund_files(out2) == ["nucl_merged_sharecov.txt", "prot_merged_otu_abund.txt"]
    assert open(out2 / "tmp" / "cp.txt").read().splitlines() == [f"{i}\tdone" for i in range(6 + 3)]
    otu = ta.read_otu(str(out2 / "contigs" / "rplB" / "prot_merged_otu_abund.txt"))
    assert all(r["ref"] is None and r["identity"] == "0.0000" and r["chimera"] == "-" for r in otu)
    assert sum(r["mass"] for r in otu) == sum(r["mass"] for r in ta.read_sharecov(str(out2 / "contigs" / "rplB" / "nucl_merged_sharecov.txt")))
    for f in ("prot_merged.fasta", "nucl_merged.fasta", "prot_merged_clust.txt"):
        assert open(out2 / "contigs" / "rplB" / f).read() == open(out / "contigs" / "rplB" / f).read()
