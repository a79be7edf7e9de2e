"""The graphs a `megagta serve` worker keeps between steps: one policy for every step that wants a graph (session.cpp).

One worker is sent matchreads A, samplecov A, coverage A, pileup A, sharecov A, matchreads B, coverage A.  Read off the code of the
commit before the policy was written once (three copies in matchreads / samplecov / pileup and `counted_graph`):
  1 matchreads A   nothing resident: loads A without multiplicities and keeps it as the match graph
  2 samplecov A    any graph will do: the match graph, "graph A: still on the device"
  3 coverage A     needs the multiplicities: drops the match graph, "load with multiplicities", keeps the counted graph
  4 pileup A       any graph will do: the counted graph, under the plain line
  5 sharecov A     the counted graph, "graph A with multiplicities: still on the device"
  6 matchreads B   other files: drops everything and loads B
  7 coverage A     loads A again: the load of B has dropped the counted graph
and run on that commit's binary before it was run on this one.  Every file of every step equals the one-shot run of the same command."""
import os
import subprocess

import numpy as np
import pytest

from megagta_amd import readlib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "megagta_amd", "bin", "megagta")
DNA = "ACGT"
FILES = {"matchreads": ["_match_reads.fa"], "samplecov": ["_samplecov.txt"], "coverage": ["_coverage.txt", "_abundance.txt"],
         "pileup": ["_pileup.txt", "_pileup_variants.txt"], "sharecov": ["_sharecov.txt"]}


def argv_of(cmd, graph, lib, fa, out):
    return [cmd, graph] + ([lib] if cmd in ("matchreads", "samplecov", "pileup") else []) + [fa, out]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """400 reads of 100 bases from a 3 kb genome (odd ones reverse-complemented, a few with one changed base), ten contigs cut from the
    genome, the graph of the reads at k = 21 (A) and, in another directory, at k = 25 (B); the seven steps one-shot and in one worker"""
    assert os.path.exists(BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    d = tmp_path_factory.mktemp("cache_policy")
    rng = np.random.default_rng(7)
    genome = rng.integers(0, 4, 3000).astype(np.uint8)
    reads = []
    for i in range(400):
        p = int(rng.integers(0, 3000 - 100 + 1))
        r = genome[p:p + 100].copy()
        if i % 9 == 0:
            r[50] = (r[50] + 1) % 4
        reads.append((3 - r)[::-1].copy() if i % 2 else r)
    lib = str(d / "reads.lib")
    parts = []
    for r in reads:                                                       # reads.lib.bin: per read uint32 length + ceil(length / 16) words
        parts += [np.array([r.size], dtype=np.uint32), readlib.pack_codes(r)]
    np.concatenate(parts).tofile(lib + ".bin")
    open(lib + ".lib_info", "w").write(f"{100 * len(reads)} {len(reads)}\nsynthetic.fa\n0 {len(reads) - 1} 100 se\n")
    fa = str(d / "contigs.fa")
    text = "".join(DNA[c] for c in genome)
    open(fa, "w").write("".join(f">contig_{j} len\n{text[280 * j:280 * j + 150 + 13 * j]}\n" for j in range(10)))
    os.mkdir(d / "other")
    A, B = str(d / "21"), str(d / "other" / "25")
    for prefix, k in ((A, 21), (B, 25)):
        r = subprocess.run([BIN, "buildgraph", "-k", str(k), "-m", "1", "--host_mem", "1e9", "--output_prefix", prefix, "--num_cpu_threads", "4",
                            "--num_output_threads", "1", "--read_lib_file", lib], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and os.path.exists(prefix + ".sdbg_info"), r.stderr[-2000:]
    steps = [("matchreads", A), ("samplecov", A), ("coverage", A), ("pileup", A), ("sharecov", A), ("matchreads", B), ("coverage", A)]
    for i, (cmd, g) in enumerate(steps):
        r = subprocess.run([BIN] + argv_of(cmd, g, lib, fa, str(d / f"one{i}")), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
    req = "".join("\t".join(argv_of(cmd, g, lib, fa, str(d / f"w{i}"))) + "\n" for i, (cmd, g) in enumerate(steps)) + "quit\n"
    w = subprocess.run([BIN, "serve"], input=req, capture_output=True, text=True, timeout=120)
    return dict(d=d, A=A, B=B, steps=steps, worker=w)


def test_every_step_is_done_and_writes_the_one_shot_files(run):
    w, d = run["worker"], run["d"]
    assert w.returncode == 0 and w.stdout.split() == ["DONE", "0"] * 7, w.stderr[-3000:]
    for i, (cmd, _) in enumerate(run["steps"]):
        for suffix in FILES[cmd]:
            one, got = open(d / f"one{i}{suffix}", "rb").read(), open(d / f"w{i}{suffix}", "rb").read()
            assert one == got and len(one) > 0, (i, cmd, suffix)
    # the inputs do what they were made for: reads match, the second coverage of A is the first, every contig has its line
    assert open(d / "one0_match_reads.fa").read().count(">") > 100
    assert open(d / "one2_coverage.txt", "rb").read() == open(d / "one6_coverage.txt", "rb").read()
    assert len(open(d / "one3_pileup.txt").read().splitlines()) >= 10


def test_the_worker_keeps_and_drops_graphs_by_the_one_policy(run):
    A, B = run["A"], run["B"]
    lines = run["worker"].stderr.splitlines()
    ends = [i for i, line in enumerate(lines) if "Real:" in line]          # every step ends with its resource line
    assert len(ends) == 7, run["worker"].stderr[-3000:]
    seg = ["\n".join(lines[(ends[i - 1] + 1 if i else 0):ends[i] + 1]) for i in range(7)]
    plain = lambda p: f"graph {p}: still on the device"
    counted = lambda p: f"graph {p} with multiplicities: still on the device"
    loads = lambda s: s.count("Number of Edges: ") == 1 and "still on the device" not in s
    # 1: the first request loads, without multiplicities
    assert loads(seg[0]) and "(load with multiplicities" not in seg[0] and "K value: 21 (load " in seg[0]
    # 2: the match graph serves samplecov
    assert seg[1].count(plain(A)) == 1 and "with multiplicities" not in seg[1] and "K value: 21 (load " in seg[1]
    # 3: coverage wants the counts: a load
    assert loads(seg[2]) and "K value: 21 (load with multiplicities " in seg[2]
    # 4, 5: the counted graph serves both, each under its own line
    assert seg[3].count(plain(A)) == 1 and "with multiplicities" not in seg[3]
    assert seg[4].count(counted(A)) == 1 and plain(A) not in seg[4] and "(load with multiplicities " in seg[4]
    # 6: other files: a load of B
    assert loads(seg[5]) and "K value: 25 (load " in seg[5] and "with multiplicities" not in seg[5]
    # 7: A again: loading B has dropped the counted graph
    assert loads(seg[6]) and "K value: 21 (load with multiplicities " in seg[6]
    # the library was read once
    assert [("library: still in memory" in s) for s in seg] == [False, True, False, True, False, True, False]
    assert B not in "".join(seg[:5]) and plain(B) not in run["worker"].stderr and counted(B) not in run["worker"].stderr
