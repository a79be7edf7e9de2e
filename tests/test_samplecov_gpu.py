"""Per-library coverage (mgta_contig_sample_coverage), `megagta samplecov` and `megagta.py --sample-abund` on the device.

Expected values never come from the code under test.  The graph is the `-m 1` graph of exactly the reads of the call, so a (k+1)-mer
has an edge iff it occurs in a read on either strand.  Per library the (k+1)-mers of the reads, each read as sequenced, are counted in a
collections.Counter; then for a window w of a contig
    count(w, s) = C_s[w] + C_s[revcomp(w)]   (C_s[w] alone where w is its own reverse complement),
    share(w)    = the number of windows of the call equal to w as strings, 0 when w is in no read or holds another letter,
    mass        = sum of (count << 16) // share, in Python integers.
The second witness does not count strings: the sum of the counts over the libraries is the uncapped multiplicity the oracle's edge
stream carries for the oracle's edge of the window, and with one library over all reads the masses are contig_share_coverage's."""
import ctypes as C
import os
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

from megagta_amd import cluster as clustlib
from megagta_amd import coverage as cv
from megagta_amd import readlib, synth
from megagta_amd import samplecov as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "megagta_amd", "bin", "megagta")
DRIVER = os.path.join(ROOT, "megagta_amd", "megagta.py")
DNA = "ACGT"
COMP = str.maketrans("ACGTacgt", "TGCAtgca")
FIELDS = ("mass", "len", "n_windows", "n_covered", "n_unique", "max_share")
LIB_END = [1, 1, 700, 1337]                                               # + the number of reads: a one-read library, an empty one, ends that are no multiple of 8 or 16
KEYS = ("mass", "contigs", "per_window_count", "per_window_share", "lib_hit_windows")


def rc(s):
    return s.translate(COMP)[::-1]


def codes(s):
    return np.array([DNA.index(c) for c in s], dtype=np.uint8)


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


def make_reads(k, seed=21):
    """1500 reads of 100 bp from a random 5 kb genome, half of them reverse-complemented; one 100 bp read 300 times, 100 side by side in
    each of three libraries; four reads shorter than k + 1; at k = 45 one 46-mer that is its own reverse complement planted in five
    reads of three libraries.  -> (reads as strings, the hot read, the planted window or None)"""
    rng = np.random.default_rng(seed)
    genome = "".join(DNA[c] for c in rng.integers(0, 4, 5000))
    base = []
    for i in range(1500):
        p = int(rng.integers(0, 5000 - 100 + 1))
        base.append(rc(genome[p:p + 100]) if i % 2 else genome[p:p + 100])
    pal = None
    if k % 2:                                                             # k + 1 even: a window can be its own reverse complement
        half = "".join(DNA[c] for c in rng.integers(0, 4, (k + 1) // 2))
        pal = half + rc(half)
        assert pal == rc(pal) and len(pal) == k + 1
        for i, at in ((0, 0), (5, 17), (650, 100 - k - 1), (651, 30), (1400, 9)):
            base[i] = base[i][:at] + pal + base[i][at + k + 1:]
            assert len(base[i]) == 100
    hot = "".join(DNA[c] for c in rng.integers(0, 4, 100))
    short = [genome[7:7 + k], genome[90:95], genome[300:300 + k - 3], ""]
    reads = base[:300] + [hot] * 100 + base[300:800] + short + [hot] * 100 + base[800:] + [hot] * 100
    return reads, hot, pal


def contig_set(strs, a, k, seed, pal):
    """about 45 contigs: test_taxonabund_gpu.py's recipe around the hot read `a` (shares 3, 4 and 7), and the pairs of a contig with its
    own reverse complement in one call"""
    rng = np.random.default_rng(seed)
    long_reads = [s for s in dict.fromkeys(strs) if len(s) >= k + 40 and s != a and (pal is None or pal not in s)]
    pick = lambda: long_reads[int(rng.integers(0, len(long_reads)))]
    out = [a, pick(), a, pick(), a]                                       # one contig three times, not side by side
    out += [a[5:k + 50], a[20:k + 40], a[20:k + 40], a[20:k + 40]]        # pieces of it: shares 3 + 1 + 3 = 7 inside, 4 around, 3 outside
    b = pick()
    out += [b, b[3:k + 30]]                                               # a contig and a piece of it
    x = pick()[:k + 12]
    out += [x + x, x[:k + 5] + x[:k + 5] + x[:k + 5]]                     # internal repeats longer than k + 1
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
    out += [rc(pick()) for _ in range(3)] + [rc(a)]                       # the other strand; the hot read with its own reverse complement
    s = pick()
    out += [s, rc(s), rc(s)[4:k + 30]]                                    # a contig, its reverse complement and a piece of that: the partner-slot case
    out.append(strs[0][10:k + 45])                                        # a piece of the first read: the one-read library counts somewhere
    if pal is not None:
        s = pick()
        out.append(s[:30] + pal + s[30:50])                               # the window that is its own reverse complement, in one contig
    while len(out) < 45:
        out.append(pick())
    return out


def restate(strs, lib_end, seqs, k):
    """the whole result of contig_sample_coverage(reads, lib_end, seqs, per_window=True) by counting strings, in Python integers"""
    n_libs = len(lib_end)
    per_lib, first = [], 0
    for end in lib_end:
        per_lib.append(Counter(s[p:p + k + 1] for s in strs[first:end] for p in range(len(s) - k)))
        first = end
    in_reads = set()
    for s in dict.fromkeys(strs[:lib_end[-1]]):
        for t in (s, rc(s)):
            in_reads.update(t[p:p + k + 1] for p in range(len(t) - k))
    wins = [[s[p:p + k + 1].upper() for p in range(len(s) - k)] for s in seqs]
    share = Counter(w for ws in wins for w in ws if w in in_reads)        # (a window with an N is in no read)
    rows, mass, pwc, pws = [], [], [], []
    for s, ws in zip(seqs, wins):
        m = [0] * n_libs
        cov = []
        for w in ws:
            sh = share.get(w, 0)
            cnt = [(c[w] + (c[rc(w)] if rc(w) != w else 0)) if sh else 0 for c in per_lib]
            for j, c in enumerate(cnt):
                if c:
                    m[j] += (c << 16) // sh
            if any(cnt):
                cov.append(sh)
            pwc.append(cnt)
            pws.append(sh)
        mass.append(m)
        rows.append(dict(mass=sum(m), len=len(s), n_windows=len(ws), n_covered=len(cov), n_unique=sum(c == 1 for c in cov), max_share=max(cov, default=0)))
    keys = {w for ws in wins for w in ws if w in in_reads}
    keys |= {rc(w) for w in keys}
    hits = [sum(n for w, n in c.items() if w in keys) for c in per_lib]
    return dict(rows=rows, mass=mass, per_window_count=pwc, per_window_share=pws, lib_hit_windows=hits, n_keys=len(keys), wins=wins,
                read_windows=[sum(c.values()) for c in per_lib])


def check_result(res, want):
    got = [{f: int(c[f]) for f in FIELDS} for c in res["contigs"]]
    for i, (g, w) in enumerate(zip(got, want["rows"])):
        assert g == w, (i, g, w)
    assert len(got) == len(want["rows"])
    assert res["mass"].tolist() == want["mass"]
    assert res["per_window_share"].tolist() == want["per_window_share"]
    assert res["per_window_count"].tolist() == want["per_window_count"]
    assert res["lib_hit_windows"].tolist() == want["lib_hit_windows"]
    st = res["stats"]
    assert st["n_keys"] == want["n_keys"] and st["n_hit_windows"] == sum(want["lib_hit_windows"]) and st["n_read_windows"] == sum(want["read_windows"])
    assert st["n_contigs"] == len(got) and st["n_windows"] == len(want["per_window_share"]) == int(res["window_offsets"][-1])
    assert st["total_mass"] == sum(r["mass"] for r in want["rows"]) and st["n_covered"] == sum(r["n_covered"] for r in want["rows"])


def same(a, b, what=""):
    for key in KEYS:
        assert a[key].tobytes() == b[key].tobytes(), (what, key)
    assert stable(a["stats"]) == stable(b["stats"]), what


def stable(stats):
    return {n: v for n, v in stats.items() if not n.startswith("ms_") and n != "n_batches"}


@pytest.fixture(scope="module")
def cases(ctx, oracle):
    """k = 20 and k = 45: reads, upload, the -m 1 graph built on the device, the oracle's graph, the contig set and the restatement of the
    call over it (computed once, never changed)"""
    from megagta_amd import api
    out = {}
    for k in (20, 45):
        strs, hot, pal = make_reads(k)
        reads = [codes(s) for s in strs]
        packed, start = readlib.pack_for_build(reads)
        rd = ctx.upload_reads(packed, start)
        stream = ctx.build_sdbg(rd, k)
        ost = oracle.Stream.build(packed, start, k, threads=4)
        oes = ost.edges()
        assert stream.md5() == oes.md5()
        g = api.Graph(ctx, stream, keep_multiplicity=True)
        lib_end = LIB_END + [len(strs)]
        seqs = contig_set(strs, hot, k, seed=k, pal=pal)
        out[k] = dict(k=k, g=g, rd=rd, strs=strs, reads=reads, lib_end=lib_end, seqs=seqs, pal=pal, stream=stream, og=oracle.Graph(ost), mult=oracle_mult(oes),
                      want=restate(strs, lib_end, seqs, k))
    return out


# ---- 1. every output against the count of strings -----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [20, 45])
def test_every_output_equals_the_count_of_strings(cases, k):
    c = cases[k]
    want, seqs = c["want"], c["seqs"]
    # the inputs hold what they were made to hold
    sh, cnt = want["per_window_share"], want["per_window_count"]
    assert {3, 4, 7} <= set(sh) and 0 in sh and {len(s) for s in seqs} >= {0, k, k + 1}
    assert any(sum(x) >= 300 and min(x[2:]) >= 100 and x[0] == x[1] == 0 for x in cnt)          # the hot read: a hundred in each of three libraries
    assert all(x[1] == 0 for x in cnt) and any(x[0] for x in cnt)                                # the empty library; the one-read library
    assert any((x << 16) % s for row, s in zip(cnt, sh) if s for x in row)                       # the floor bites somewhere
    assert want["read_windows"][1] == 0 and any(len(s) <= k for s in c["strs"])
    if c["pal"]:
        flat = [w for ws in want["wins"] for w in ws]
        assert flat.count(c["pal"]) == 1 and sum(cnt[flat.index(c["pal"])]) == 5 and sh[flat.index(c["pal"])] == 1       # once per read window
    res = c["g"].contig_sample_coverage(c["rd"], c["lib_end"], seqs, per_window=True)
    check_result(res, want)
    # without the per-window outputs: the same records; n = 0
    r1 = c["g"].contig_sample_coverage(c["rd"], c["lib_end"], seqs)
    assert r1["per_window_count"] is None and r1["per_window_share"] is None
    assert r1["contigs"].tobytes() == res["contigs"].tobytes() and r1["mass"].tobytes() == res["mass"].tobytes()
    r0 = c["g"].contig_sample_coverage(c["rd"], c["lib_end"], [], per_window=True)
    assert r0["contigs"].size == 0 and r0["mass"].size == 0 and all(v == 0 for v in r0["stats"].values()) and not r0["lib_hit_windows"].any()


# ---- 2. the second witness: the oracle's multiplicities, and the pooled call ---------------------------------------------------------
@pytest.mark.parametrize("k", [20, 45])
def test_counts_sum_to_the_multiplicity_and_one_library_is_the_pooled_mass(cases, k):
    c = cases[k]
    res = c["g"].contig_sample_coverage(c["rd"], c["lib_end"], c["seqs"], per_window=True)
    total = res["per_window_count"].sum(axis=1)
    wins = [w for ws in c["want"]["wins"] for w in ws]
    assert len(wins) == total.size
    checked = 0
    for w, t in zip(wins, total.tolist()):
        if w == rc(w):
            continue
        e = c["og"].index_edge(w) if set(w) <= set(DNA) else -1
        assert t == (int(c["mult"][e]) if e >= 0 else 0), w
        checked += e >= 0
    assert checked > 1000 and int(c["mult"].max()) < 65535
    one = c["g"].contig_sample_coverage(c["rd"], [len(c["strs"])], c["seqs"], per_window=True)
    pooled = c["g"].contig_share_coverage(c["seqs"], per_window=True)
    not_pal = np.array([w != rc(w) for w in wins])
    assert np.array_equal(one["per_window_share"], pooled["per_window_share"])
    assert np.array_equal(one["per_window_count"][:, 0][not_pal], pooled["per_window"][not_pal].astype(np.uint64))
    if not c["pal"]:
        assert one["mass"][:, 0].tolist() == pooled["contigs"]["mass"].tolist()
        assert one["contigs"].tobytes() == pooled["contigs"].tobytes()
    else:                                                                 # (the graph counts a read window that is its own reverse complement on both strands)
        clean = [i for i, ws in enumerate(c["want"]["wins"]) if c["pal"] not in ws]
        assert len(clean) == len(c["seqs"]) - 1
        assert one["mass"][clean, 0].tolist() == pooled["contigs"]["mass"][clean].tolist()
    # the sum over the libraries is within n_libs units per covered window of the pooled mass
    many = res["mass"].sum(axis=1).astype(np.int64) - one["mass"][:, 0].astype(np.int64)
    assert (many <= 0).all() and (-many <= len(c["lib_end"]) * res["contigs"]["n_covered"].astype(np.int64)).all()


# ---- 3. what must not move the outputs ------------------------------------------------------------------------------------------------
def test_batches_collisions_repetition_and_other_calls_move_no_output(cases):
    c = cases[20]
    g, rd, ends, seqs = c["g"], c["rd"], c["lib_end"], c["seqs"]
    a = g.contig_sample_coverage(rd, ends, seqs, per_window=True)
    b = g.contig_sample_coverage(rd, ends, seqs, per_window=True)          # no marks or counts left over
    same(a, b, "twice")
    g.match_reads(rd, seqs[:7], counts=True)
    g.contig_coverage(seqs[:9], abundance=True)
    same(a, g.contig_sample_coverage(rd, ends, seqs, per_window=True), "after match_reads and contig_coverage")
    runs = {}
    for what, batch, bits in (("batch", 64, 64), ("bits", 0, 4), ("both", 64, 4)):
        g.ctx.set_coverage_batch(batch)
        g.ctx.set_share_hash_bits(bits)
        try:
            runs[what] = g.contig_sample_coverage(rd, ends, seqs, per_window=True)
        finally:
            g.ctx.set_coverage_batch(0)
            g.ctx.set_share_hash_bits(64)
    assert a["stats"]["n_batches"] == 1 and runs["batch"]["stats"]["n_batches"] > 5 and runs["bits"]["stats"]["n_batches"] == 1
    for what, r in runs.items():
        same(a, r, what)
    check_result(runs["both"], c["want"])


@pytest.mark.parametrize("k", [20, 45])
def test_read_order_inside_a_library_and_storage_order_move_no_output(ctx, cases, k):
    c = cases[k]
    g, ends, seqs = c["g"], c["lib_end"], c["seqs"]
    a = g.contig_sample_coverage(c["rd"], ends, seqs, per_window=True)
    rng = np.random.default_rng(3)
    order, first = [], 0
    for end in ends:
        order += (first + rng.permutation(end - first)).tolist()
        first = end
    assert order != list(range(len(order))) and sorted(order) == list(range(len(order)))
    shuffled = [c["reads"][i] for i in order]
    rd2 = ctx.upload_reads(*readlib.pack_for_build(shuffled))
    r = g.contig_sample_coverage(rd2, ends, seqs, per_window=True)
    rd2.free()
    for key in KEYS:
        assert a[key].tobytes() == r[key].tobytes(), key
    assert stable(a["stats"]) == stable(r["stats"])                       # (where the walk of a read has to start again does not depend on the order either)
    # stored as sequenced
    lens = np.array([x.size for x in c["reads"]], dtype=np.uint64)
    start = np.zeros(lens.size + 1, dtype=np.uint64)
    np.cumsum(lens, out=start[1:])
    rd3 = ctx.upload_reads(readlib.pack_codes(np.concatenate(c["reads"])), start)
    f = g.contig_sample_coverage(rd3, ends, seqs, per_window=True, reads_reversed=False)
    rd3.free()
    for key in KEYS:
        assert a[key].tobytes() == f[key].tobytes(), key
    # reads behind the last end are not scanned
    cut = g.contig_sample_coverage(c["rd"], ends[:-1], seqs, per_window=True)
    assert cut["per_window_count"].tobytes() == a["per_window_count"][:, :-1].tobytes() and cut["stats"]["n_reads"] == ends[-2]


# ---- 4. errors ------------------------------------------------------------------------------------------------------------------------
def test_guards_write_nothing(cases):
    from megagta_amd import api
    c = cases[20]
    g, rd = c["g"], c["rd"]
    L = g.ctx._L
    off = np.array([0, 40], dtype=np.uint64)
    mass = np.full(300, 0xAB, dtype=np.uint64)
    hits = np.full(300, 0xAB, dtype=np.uint64)
    rec = np.full(64, 0xAB, dtype=np.uint8)
    st = api._lib.SampleCovStats()

    def call(graph, reads, ends, n_libs, m=mass, offsets=off, n=1):
        e = np.array(ends, dtype=np.uint64)
        return L.mgta_contig_sample_coverage(graph, reads, 1, e.ctypes.data if e.size else None, n_libs, b"A" * 40, offsets.ctypes.data, n,
                                             m.ctypes.data if m is not None else None, rec.ctypes.data, None, None, hits.ctypes.data, C.byref(st))

    n = rd.n_reads
    assert call(g.h, rd.h, [n], 0) == -1 and b"n_libs = 0" in L.mgta_last_error()
    assert call(g.h, rd.h, [n] * 257, 257) == -1 and b"n_libs = 257" in L.mgta_last_error() and b"256" in L.mgta_last_error()
    assert call(g.h, rd.h, [5, 4, n], 3) == -1 and b"descend" in L.mgta_last_error()
    assert call(g.h, rd.h, [5, n + 1], 2) == -1 and b"reads" in L.mgta_last_error()
    assert call(g.h, rd.h, [n], 1, m=None) == -1 and b"mass" in L.mgta_last_error()
    assert call(None, rd.h, [n], 1) == -1 and call(g.h, None, [n], 1) == -1
    big = 0xFFFFFFF0
    assert call(g.h, rd.h, [n], 1, offsets=np.array([0, big, 2 * big], dtype=np.uint64), n=2) == -1 and b"2^32" in L.mgta_last_error()
    assert call(g.h, rd.h, [n], 1, n=1 << 31) == -1 and b"2^31" in L.mgta_last_error()
    other = api.Context(0)
    try:
        rd2 = other.upload_reads(*readlib.pack_for_build(c["reads"][:50]))
        with pytest.raises(api.MegaGtaError, match=r"\(-1\).*different contexts"):
            g.contig_sample_coverage(rd2, [50], ["A" * 40])
        rd2.free()
    finally:
        other.close()
    assert (mass == 0xAB).all() and (hits == 0xAB).all() and (rec == 0xAB).all()
    assert call(g.h, rd.h, [n], 1) == 0 and mass[0] == 0 and (mass[1:] == 0xAB).all()       # (the same arguments within the limits are a valid call)


# ---- 5. the command, the worker and the driver ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run_inputs(golden_dir, tmp_path_factory):
    """~2000 reads of the driver tests' sample in two files: two libraries"""
    d = tmp_path_factory.mktemp("two_libs")
    mg = synth.make_metagenome(2000, 150, (("rplB", 100),), seed=11, reads_per_genome=1000)
    synth.write_fasta(mg.reads[:1203], str(d / "a.fa"))
    synth.write_fasta(mg.reads[1203:], str(d / "b.fa"))
    toy = os.path.join(golden_dir, "toy")
    (d / "gene_list.txt").write_text(f"rplB {toy}/for_enone.hmm {toy}/rev_enone.hmm {toy}/ref_aligned.faa\n")
    base = [sys.executable, DRIVER, "-r", str(d / "a.fa"), "-r", str(d / "b.fa"), "-g", str(d / "gene_list.txt"), "-k", "21", "-t", "4", "--min-contig-len", "100"]
    return d, base, mg


def new_files(out):
    return sorted(f for _, _, files in os.walk(out) for f in files if "samplecov" in f or "otu_samples" in f)


def tree(root):
    return {os.path.relpath(os.path.join(dp, f), root): open(os.path.join(dp, f), "rb").read() for dp, _, fs in os.walk(root) for f in fs}


def test_driver_sample_abund_command_and_worker(ctx, run_inputs):
    from megagta_amd import api
    tmp, base, mg = run_inputs
    out, plain = tmp / "with", tmp / "plain"
    for o, extra in ((out, ["--sample-abund"]), (plain, [])):
        r = subprocess.run(base + ["-o", str(o), "--derep", "--align", "--cluster"] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr + open(o / "log").read()[-2000:]
    d = out / "contigs" / "rplB"
    assert new_files(out) == ["nucl_merged_rmdup_samplecov.txt", "prot_merged_rmdup_otu_samples.txt", "prot_merged_rmdup_otu_samples_ppm.txt"] and new_files(plain) == []
    # a run without the flag: the same files and checkpoints, minus the new files and their checkpoint
    ta, tb = tree(str(out)), tree(str(plain))
    assert set(ta) - set(tb) == {"contigs/rplB/" + f for f in new_files(out)} and set(tb) <= set(ta)
    for f in set(tb) - {"log", "opts.txt", "tmp/cp.txt"}:
        assert ta[f] == tb[f], f
    cp_a, cp_b = ta["tmp/cp.txt"].decode().splitlines(), tb["tmp/cp.txt"].decode().splitlines()
    assert cp_b == [f"{i}\tdone" for i in range(len(cp_b))] and cp_a == cp_b + [f"{len(cp_b)}\tdone"]
    assert "every library" not in tb["log"].decode() and "samplecov" not in tb["log"].decode()
    log = ta["log"].decode()
    assert log.index("Clustering the aligned contigs") < log.index("Counting the reads of every library on the contigs of rplB") < log.index("Summing the clusters of rplB per library")
    # the coverage file: the API's numbers on the run's graph and library, in the writer's bytes
    lib = str(out / "tmp" / "reads.lib")
    table = readlib.read_lib_table(lib)
    assert [(t[1], t[2], t[4]) for t in table] == [(0, 1202, False), (1203, 1999, False)]
    ends = [t[2] + 1 for t in table]
    names, seqs = cv.read_fasta(str(d / "nucl_merged_rmdup.fasta"))
    assert len(names) >= 1
    packed, start = readlib.load_for_build(lib)
    g = api.Graph.from_files(ctx, str(out / "k20" / "20"))
    rd = ctx.upload_reads(packed, start)
    res = g.contig_sample_coverage(rd, ends, seqs)
    libs = sc.libs_of(table, sc.lib_read_windows(start, ends, 20), res["lib_hit_windows"])
    text = sc.samplecov_text(libs, names, res["contigs"], res["mass"])
    assert text.encode() == ta["contigs/rplB/nucl_merged_rmdup_samplecov.txt"]
    assert [x["reads"] for x in libs] == [1203, 797] and [x["read_windows"] for x in libs] == [1203 * 130, 797 * 130] and all(x["hit_windows"] > 0 for x in libs)
    # ... and by counting strings: the contigs of the search are paths of this very graph, every window of theirs is in a read
    strs = ["".join(DNA[c] for c in r) for r in mg.reads]
    want = restate(strs, ends, seqs, 20)
    assert res["mass"].tolist() == want["mass"] and res["lib_hit_windows"].tolist() == want["lib_hit_windows"]
    assert [{f: int(c[f]) for f in FIELDS} for c in res["contigs"]] == want["rows"] and all(r["n_covered"] == r["n_windows"] for r in want["rows"])
    # the tables are the join of the two files and add up
    cov = sc.read_samplecov(str(d / "nucl_merged_rmdup_samplecov.txt"))
    otu = sc.read_otu_samples(str(d / "prot_merged_rmdup_otu_samples.txt"))
    ppm = sc.read_otu_samples_ppm(str(d / "prot_merged_rmdup_otu_samples_ppm.txt"))
    joined = sc.join(cov, clustlib.read_clust(str(d / "prot_merged_rmdup_clust.txt")))
    assert sc.otu_samples_text(joined).encode() == ta["contigs/rplB/prot_merged_rmdup_otu_samples.txt"]
    assert sc.otu_samples_ppm_text(joined).encode() == ta["contigs/rplB/prot_merged_rmdup_otu_samples_ppm.txt"]
    for s in range(2):
        assert sum(r["mass"][s] for r in otu["rows"]) == otu["total"][s] == sum(r["mass"][s] for r in cov["rows"]) > 0
        assert sum(r["mass"][s] for r in ppm["rows"]) <= 1000000
    assert otu["records"] == len(names) and otu["libs"] == cov["libs"] == libs
    # the command alone, and as requests to the worker by matchreads' rules for what it keeps
    fa = str(d / "nucl_merged_rmdup.fasta")
    prefix = str(out / "k20" / "20")
    subprocess.run([BIN, "samplecov", prefix, lib, fa, str(tmp / "one")], check=True, capture_output=True, timeout=120)
    assert open(tmp / "one_samplecov.txt").read() == text
    req = f"matchreads\t{prefix}\t{lib}\t{fa}\t{tmp}/w\nsamplecov\t{prefix}\t{lib}\t{fa}\t{tmp}/w\nsamplecov\t{prefix}\t{lib}\t{fa}\t{tmp}/w2\nquit\n"
    r = subprocess.run([BIN, "serve"], input=req, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["DONE", "0"] * 3, r.stderr[-2000:]
    assert r.stderr.count(f"graph {prefix}: still on the device") == 2 and r.stderr.count("library: still in memory") == 2
    assert open(tmp / "w_samplecov.txt").read() == text == open(tmp / "w2_samplecov.txt").read()
    r = subprocess.run([BIN, "samplecov", prefix, lib, fa], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Usage: megagta samplecov" in r.stderr
    rd.free()
    g.free()
    # --continue on the finished run skips the finished genes
    before = ta["contigs/rplB/prot_merged_rmdup_otu_samples.txt"]
    r = subprocess.run([sys.executable, DRIVER, "--continue", "-o", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and open(d / "prot_merged_rmdup_otu_samples.txt", "rb").read() == before
    assert open(out / "log").read().count("Counting the reads of every library") == 1
