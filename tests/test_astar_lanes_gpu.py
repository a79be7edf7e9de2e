"""A* search batches on a context that is not the graph's own (mgta_astar_batch_on), under a share of the CUs
(mgta_ctx_set_search_share), and two of them side by side -- the route `megagta search` takes with MEGAGTA_SEARCH_LANES=2, and what
include/megagta_hip.h promises for it: "Results do not depend on it."
Yardsticks: the reference's per-seed goldens of the toy graph (cold) and the oracle's sequential restatement of the sharing rule (the
shared-cache modes), as in tests/test_astar_gpu.py; on top of them every run must equal, bit for bit, the same batch on the graph's own
context without a share."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import threading
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                                             # (the child of test_two_batches_side_by_side starts from this file)
    sys.path.insert(0, ROOT)

from megagta_amd import search_dist, synth                          # noqa: E402
from tests import helpers as H                                       # noqa: E402
from tests import test_astar_gpu as TA                               # noqa: E402
from tests.test_astar_gpu import _check_side, ctx, meta20k, toy      # noqa: E402,F401  (the fixtures of the A* suite, as they are)

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden")
BIN = os.path.join(ROOT, "megagta_amd", "bin", "megagta")
SHARES = [(1, 1), (1, 2), (1, 3), (1, 16), (1, 4096)]               # (1, 4096): the floor of two workgroups, one per direction
SLACK = 512 << 20                                                    # what the device's free-memory figure may move by on its own (the pools are 4 GB and more)


@pytest.fixture(scope="module")
def ctx_b(ctx):
    """context B: created on device 0 next to the graphs' context A"""
    from megagta_amd import api
    c = api.Context(0)
    yield c
    c.close()


# ---- the batches and their yardsticks -------------------------------------------------------------------------------------------------
def _side_ref(o):
    """an oracle side as the records `_check_side` compares with (the goldens' names)"""
    return dict(ok=o.ok, real=o.real_score, score=o.score, fval=o.fval, length=o.length, state_no=o.state_no, state=chr(o.state), node=o.node_id,
                closed=o.n_closed, expanded=o.n_expanded)


_oracle_runs = {}


def _oracle_refs(oracle, meta, cache_mode, cost_rate, lo=0, hi=400):
    """the oracle's results for seeds [lo, hi) of meta20k as ONE batch (a cache of its own): cold, or run one after the other under the
    sharing rule (window, cost rate) -> [dict(contig, R, L)], once per module"""
    key = (cache_mode, cost_rate, lo, hi)
    if key not in _oracle_runs:
        S = oracle.Searcher(meta.oracle_graph(oracle), oracle.Hmm(meta.fpath), oracle.Hmm(meta.rpath), 20, 0.5)
        S.clear_cache()
        if cache_mode:
            S.set_window(cache_mode)
            S.set_cost_rate(cost_rate)
        out = []
        for kmer, pos in meta.seeds[lo:hi]:
            contig, R, L = S.search(kmer, pos - 1, cold=cache_mode == 0)
            out.append(dict(contig=contig, R=_side_ref(R), L=_side_ref(L)))
        _oracle_runs[key] = out
    return _oracle_runs[key]


def _toy_gold(fname):
    return H.parse_probe_astar(H.gz_lines(os.path.join(GOLDEN, "toy", fname)))


BATCHES = ["toy-prune20", "toy-prune0", "meta-cold", "meta-sequential", "meta-window"]


def _batch(name, toy, meta, oracle):
    """-> (graph, fwd, rev, kmers, states, prune, cache_mode, cost_rate, refs = [dict(contig, R, L)])"""
    if name.startswith("toy"):
        g, fw, rv, _ = toy
        prune = 20 if name == "toy-prune20" else 0
        gold = _toy_gold("astar_cold.txt.gz" if prune else "astar_cold_prune0.txt.gz")
        return g, fw, rv, [r["kmer"] for r in gold], [r["start_state"] for r in gold], prune, 0, 0, gold
    cache_mode, rate = {"meta-cold": (0, 0), "meta-sequential": (1, 0), "meta-window": search_dist.window_and_rate(400)}[name]
    return meta.g, meta.fw, meta.rv, meta.kmers, meta.states, 20, cache_mode, rate, _oracle_refs(oracle, meta, cache_mode, rate)


def _check_against(res, kmers, refs):
    assert len(res) == len(refs) == len(kmers)
    for r, km, ref in zip(res, kmers, refs):
        _check_side(r.right_side, ref["R"])
        _check_side(r.left_side, ref["L"])
        if "expanded" in ref["R"]:
            assert (r.right_side["n_expanded"], r.left_side["n_expanded"]) == (ref["R"]["expanded"], ref["L"]["expanded"])
        assert r.contig(km) == ref["contig"]


def _same(res, want, kmers):
    for a, b, km in zip(res, want, kmers):
        assert a.contig(km) == b.contig(km) and a.right_side == b.right_side and a.left_side == b.left_side


# ---- a. a second context alone, under every share ----------------------------------------------------------------------------------------
_on_a = {}


def _run_on_a(name, group, toy, meta, oracle):
    """the batch on the graph's own context A without a share, checked against its yardstick: once per module, batch and lane grouping
    (the caller has set MGTA_ASTAR_GROUP)"""
    from megagta_amd import api
    if (name, group) not in _on_a:
        g, fw, rv, kmers, states, prune, mode, rate, refs = _batch(name, toy, meta, oracle)
        want, st0 = api.astar_search(g, fw, rv, kmers, states, prune, 0.5, cache_mode=mode, cost_rate=rate)
        _check_against(want, kmers, refs)
        assert st0["n_retries"] == 0 and st0["n_over_limit"] == 0 and st0["n_seeds"] == len(kmers)
        _on_a[name, group] = (want, st0)
    return _on_a[name, group]


@pytest.mark.parametrize("share", SHARES, ids=lambda s: f"{s[0]}of{s[1]}")
@pytest.mark.parametrize("group", [16, 64])
@pytest.mark.parametrize("name", BATCHES)
def test_second_context_under_every_share(ctx, ctx_b, toy, meta20k, oracle, monkeypatch, name, group, share):
    """the batch on B -- its stream, pool, meta words and events; A's graph -- under no share, a half, a third, a sixteenth and the floor of
    two workgroups: the reference's goldens (toy, cold) or the oracle's restatement (meta20k: cold, sequential, the plan's window), and bit
    for bit the run on A"""
    from megagta_amd import api
    monkeypatch.setenv("MGTA_ASTAR_GROUP", str(group))
    g, fw, rv, kmers, states, prune, mode, rate, refs = _batch(name, toy, meta20k, oracle)
    want, st0 = _run_on_a(name, group, toy, meta20k, oracle)
    try:
        ctx_b.set_search_share(*share)
        res, st = api.astar_search(g, fw, rv, kmers, states, prune, 0.5, cache_mode=mode, cost_rate=rate, run=ctx_b)
    finally:
        ctx_b.set_search_share(1, 1)
    _check_against(res, kmers, refs)
    _same(res, want, kmers)
    assert (st["n_seeds"], st["n_expansions"], st["n_opened"]) == (st0["n_seeds"], st0["n_expansions"], st0["n_opened"])
    assert st["n_retries"] == 0 and st["n_over_limit"] == 0, st


# ---- b. the share is really applied -----------------------------------------------------------------------------------------------------
def _per_device(stats):
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * (1 if stats["hmm_in_lds"] else 2)


def _expected_workgroups(baseline, per_device, num, den):
    """plan_pass (astar.hip) restated: the smaller of the grid the work asks for and the context's share of the device -- at least two
    workgroups --, rounded up to an even count"""
    n = min(baseline, max(2, per_device * num // den))
    return max(2, n + (n & 1))


def _run_and_count(capfd, *args, **kw):
    """one batch with MGTA_ASTAR_VERBOSE=1 -> (results, stats, the workgroups of its pass 0 as the library printed them)"""
    from megagta_amd import api
    capfd.readouterr()
    res, st = api.astar_search(*args, **kw)
    err = capfd.readouterr().err
    n = re.findall(r"\[astar\] pass 0: (\d+) workgroups", err)
    assert len(n) == 1 and "pass 1:" not in err, err[-2000:]
    return res, st, int(n[0])


@pytest.mark.parametrize("group", [16, 64])
def test_the_share_sets_the_grid(ctx, ctx_b, meta20k, monkeypatch, capfd, group):
    """the workgroups of the pass ("pass 0: N workgroups" of MGTA_ASTAR_VERBOSE=1) are plan_pass's rule for every share; 400 cold seeds ask for
    26 workgroups (16 lanes per search) or 100 (64 lanes), so a sixteenth (16 of 256 CUs) and the floor (2) bind in both groupings, and a third
    (85, rounded up to 86) binds with 64 lanes.  A library that ignored the share would launch the unshared grid every time.  The share is
    B's alone: a batch on A meanwhile launches the unshared grid"""
    monkeypatch.setenv("MGTA_ASTAR_GROUP", str(group))
    monkeypatch.setenv("MGTA_ASTAR_VERBOSE", "1")
    m = meta20k
    args = (m.g, m.fw, m.rv, m.kmers, m.states, 20, 0.5)
    want, st0, baseline = _run_and_count(capfd, *args, run=ctx_b)
    per_device = _per_device(st0)
    assert baseline == min(per_device, 2 * -(-400 // (8 * (64 // group)))), (baseline, per_device)       # (8 waves of 64 / G searches per workgroup)
    bound = []
    try:
        for num, den in SHARES:
            ctx_b.set_search_share(num, den)
            res, st, n = _run_and_count(capfd, *args, run=ctx_b)
            expect = _expected_workgroups(baseline, per_device, num, den)
            print(f"G {group}, share {num}/{den}: {n} workgroups (unshared {baseline}, {per_device} per device)")
            assert n == expect, (num, den, n, expect, baseline, per_device)
            if expect < baseline:
                bound.append((num, den))
            _same(res, want, m.kmers)
            assert st["n_expansions"] == st0["n_expansions"]
        assert {(1, 16), (1, 4096)} <= set(bound), bound                   # (the share term binds, not the work term)
        assert ((1, 3) in bound) == (group == 64) and (1, 1) not in bound
        _, _, on_a = _run_and_count(capfd, *args)                         # (B still holds 1 / 4096)
        assert on_a == baseline
    finally:
        ctx_b.set_search_share(1, 1)


# ---- c. the work memory is the run context's ----------------------------------------------------------------------------------------------
def _free_bytes(c):
    from megagta_amd import api
    f, t = C.c_uint64(), C.c_uint64()
    api.check(c._L.mgta_ctx_device_memory(c.h, C.byref(f), C.byref(t)), "mgta_ctx_device_memory")
    return f.value


def test_the_pool_is_the_run_contexts(ctx, toy, meta20k):
    """the pool of a batch on B (4 GB at least) is B's: the device's free memory falls by it, A has nothing to give back afterwards
    (release_scratch on A frees nothing), closing B returns it, and A searches as before"""
    from megagta_amd import api
    g, fw, rv, _ = toy
    gold = _toy_gold("astar_cold.txt.gz")
    kmers, states = [r["kmer"] for r in gold], [r["start_state"] for r in gold]
    before, stb = api.astar_search(g, fw, rv, kmers, states, 20, 0.5)
    ctx.release_scratch()                                                 # (A holds its graphs and models, no work memory)
    f0 = _free_bytes(ctx)
    b = api.Context(0)
    try:
        m = meta20k
        res, st = api.astar_search(m.g, m.fw, m.rv, m.kmers, m.states, 20, 0.5, run=b)
        f1 = _free_bytes(b)
        assert st["pool_bytes"] >= 4 << 30 and st["n_retries"] == 0
        assert f0 - f1 >= st["pool_bytes"] - SLACK, (f0, f1, st["pool_bytes"])
        ctx.release_scratch()
        f2 = _free_bytes(ctx)
        assert abs(f2 - f1) < SLACK, (f1, f2)                             # (a pool on A would have come back here)
    finally:
        b.close()
    f3 = _free_bytes(ctx)
    print(f"free device memory: {f0} before, {f1} after the batch on B (pool {st['pool_bytes']}), {f2} after A released its scratch, {f3} after B closed")
    assert f3 - f2 >= st["pool_bytes"] - SLACK, (f2, f3, st["pool_bytes"])
    after, sta = api.astar_search(g, fw, rv, kmers, states, 20, 0.5)
    _same(after, before, kmers)
    _check_against(after, kmers, gold)
    assert (sta["n_expansions"], sta["n_opened"]) == (stb["n_expansions"], stb["n_opened"])


# ---- d. two batches side by side (in a child process) ------------------------------------------------------------------------------------
# Measured in the child on an MI355X, twice (the file alone; the file after the whole suite), 16 lanes per search, each context with half of
# the CUs -- wall time of the Python call, the first solo batch of the process included:
#   halves-window        (seeds 0..199 on A | 200..399 on B, the plan's window 1024 + 4): solo 0.25 + 0.27 s / 0.22 + 0.23 s, side by side 0.26 / 0.48 s
#   toy-cold|meta-window (93 toy goldens cold on B | 400 seeds windowed on A):            solo 0.13 + 0.25 s / 0.14 + 0.26 s, side by side 0.28 / 0.27 s
#   halves-window4       (window 4, 16 expansions per seed, the halves again):            solo 0.29 + 0.26 s / 0.29 + 0.28 s, side by side 0.56 / 0.30 s
# The largest sum of two solo batches is 0.57 s; a side-by-side step gets ten times that (a batch on half the CUs takes about twice as long,
# the machine is shared, the first call loads the code object).  The child as a whole -- two graphs built, six solo batches, three
# side-by-side steps -- took 3.0 s after its imports (6 s for the test); its limit is the three steps' limits plus ten times those 6 s.
SIDE_BY_SIDE_LIMIT_S = 5.7
CHILD_LIMIT_S = 3 * SIDE_BY_SIDE_LIMIT_S + 60.0


def _plain(res, kmers):
    return [[r.contig(km), r.right_side, r.left_side] for r, km in zip(res, kmers)]


def _child(out_path):
    """one graph per seed set, contexts A and B with half of the CUs each; every round runs its two batches one after the other, then at
    once from two threads behind a barrier (the ctypes calls release the GIL); results, stats and wall times go to `out_path`"""
    from megagta_amd import api
    t_start = time.time()
    a, b = api.Context(0), api.Context(0)
    tmp = tempfile.mkdtemp(prefix="lanes_child_")
    meta = TA._Meta20k(a, tmp)
    toy_g, toy_fw, toy_rv, _ = TA.toy.__wrapped__(a, GOLDEN)
    gold = _toy_gold("astar_cold.txt.gz")
    window, rate = search_dist.window_and_rate(200)
    a.set_search_share(1, 2)
    b.set_search_share(1, 2)

    def half(lo, hi, run, mode, cost):
        return dict(args=(meta.g, meta.fw, meta.rv, meta.kmers[lo:hi], meta.states[lo:hi], 20, 0.5), kw=dict(cache_mode=mode, cost_rate=cost, run=run))

    rounds = {
        "halves-window": (half(0, 200, a, window, rate), half(200, 400, b, window, rate)),
        "toy-cold|meta-window": (dict(args=(toy_g, toy_fw, toy_rv, [r["kmer"] for r in gold], [r["start_state"] for r in gold], 20, 0.5), kw=dict(run=b)),
                                 half(0, 400, a, window, rate)),
        "halves-window4": (half(0, 200, a, 4, 16), half(200, 400, b, 4, 16)),
    }
    report = dict(limit_s=SIDE_BY_SIDE_LIMIT_S, rounds={})
    for name, jobs in rounds.items():
        solo, solo_s = [], []
        for j in jobs:
            t0 = time.time()
            res, st = api.astar_search(*j["args"], **j["kw"])
            solo_s.append(time.time() - t0)
            solo.append(dict(results=_plain(res, j["args"][3]), stats=st))
        both, barrier = [None, None], threading.Barrier(2)

        def lane(i, j):
            barrier.wait()
            try:
                res, st = api.astar_search(*j["args"], **j["kw"])
                both[i] = dict(results=_plain(res, j["args"][3]), stats=st)
            except Exception as e:                                        # (reported, not lost with the thread)
                both[i] = dict(error=repr(e))

        threads = [threading.Thread(target=lane, args=(i, j), daemon=True) for i, j in enumerate(jobs)]
        t0 = time.time()
        for t in threads:
            t.start()
        for t in threads:
            t.join(max(0.0, SIDE_BY_SIDE_LIMIT_S - (time.time() - t0)))
        wall = time.time() - t0
        if any(t.is_alive() for t in threads):                            # a stall ends the child, with what it knows, and not the suite
            report["rounds"][name] = dict(stalled=True, solo_s=solo_s, side_by_side_s=wall)
            with open(out_path, "w") as f:
                json.dump(report, f)
            os._exit(3)
        report["rounds"][name] = dict(solo=solo, side_by_side=both, solo_s=solo_s, side_by_side_s=wall)
        print(f"{name}: solo {solo_s[0]:.2f} s + {solo_s[1]:.2f} s, side by side {wall:.2f} s", flush=True)
    report["child_s"] = time.time() - t_start
    print(f"child: {report['child_s']:.1f} s", flush=True)
    with open(out_path, "w") as f:
        json.dump(report, f)
    b.close()
    a.close()


class _Res:
    """a result of the child as `_check_against` reads one"""

    def __init__(self, rec):
        self._contig, self.right_side, self.left_side = rec

    def contig(self, kmer):
        return self._contig


def test_two_batches_side_by_side(meta20k, oracle, tmp_path):
    """two host threads, two contexts with half of the CUs each, one graph: every batch is byte for byte its solo run and the oracle's
    restatement over its OWN seeds (a cache of its own); a cold batch of the toy goldens beside a windowed one (two graphs, two model pairs)
    gives the reference's goldens, and the stats of each describe that batch alone.  No assertion on speed or overlap"""
    out = tmp_path / "lanes.json"
    env = {k: v for k, v in os.environ.items() if k not in ("MGTA_ASTAR_GROUP", "MGTA_ASTAR_VERBOSE")}
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], capture_output=True, text=True, timeout=CHILD_LIMIT_S, cwd=ROOT, env=env)
    print(r.stdout)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    rep = json.loads(out.read_text())
    window, rate = search_dist.window_and_rate(200)
    m = meta20k
    gold = _toy_gold("astar_cold.txt.gz")
    yardsticks = {
        "halves-window": ((m.kmers[:200], _oracle_refs(oracle, m, window, rate, 0, 200)), (m.kmers[200:], _oracle_refs(oracle, m, window, rate, 200, 400))),
        "toy-cold|meta-window": (([g["kmer"] for g in gold], gold), (m.kmers, _oracle_refs(oracle, m, window, rate, 0, 400))),
        "halves-window4": ((m.kmers[:200], _oracle_refs(oracle, m, 4, 16, 0, 200)), (m.kmers[200:], _oracle_refs(oracle, m, 4, 16, 200, 400))),
    }
    assert set(rep["rounds"]) == set(yardsticks)
    for name, rnd in rep["rounds"].items():
        assert not rnd.get("stalled"), (name, rnd)
        for solo, both, (kmers, refs) in zip(rnd["solo"], rnd["side_by_side"], yardsticks[name]):
            assert "error" not in both, both
            assert json.dumps(both["results"]) == json.dumps(solo["results"]), name
            _check_against([_Res(x) for x in both["results"]], kmers, refs)
            _check_against([_Res(x) for x in solo["results"]], kmers, refs)
            for st in (solo["stats"], both["stats"]):                       # each batch's stats are its own
                assert st["n_seeds"] == len(kmers), name
                assert st["n_expansions"] == sum(x[1]["n_expanded"] + x[2]["n_expanded"] for x in both["results"]), name
                assert st["n_opened"] == sum(x[1]["n_opened"] + x[2]["n_opened"] for x in both["results"]), name
                assert st["n_retries"] == 0 and st["n_over_limit"] == 0, (name, st)
    # (the two halves are two batches, not one cut in two: with a window that shares, the second half's searches differ from those the
    # same seeds make behind the first half's paths)
    whole = _oracle_refs(oracle, m, 4, 16, 0, 400)
    halves = _oracle_refs(oracle, m, 4, 16, 200, 400)
    assert [w["R"]["expanded"] + w["L"]["expanded"] for w in whole[200:]] != [h["R"]["expanded"] + h["L"]["expanded"] for h in halves]


# ---- e. `megagta search` with two lanes ------------------------------------------------------------------------------------------------
CLI_LIMIT_S = 300                                                        # (each process on its own; they take seconds)
GENES = ("rplB", "nirK", "nifH")


def _search(d, gene_list, tag, lanes):
    env = {k: v for k, v in os.environ.items() if k != "MEGAGTA_SEARCH_LANES"}
    if lanes is not None:
        env["MEGAGTA_SEARCH_LANES"] = lanes
    pre = str(d / "44")
    return subprocess.run([BIN, "search", pre, str(gene_list), pre, str(d / tag), "20", "0.5", "4"], capture_output=True, text=True, env=env, timeout=CLI_LIMIT_S)


@pytest.fixture(scope="module")
def cli_inputs(tmp_path_factory):
    """20 000 reads with three genes, the graph files written once, the seeds of every gene from `megagta findstart`, and the one-lane runs
    of the three-gene and the one-gene list"""
    assert os.path.exists(BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    d = tmp_path_factory.mktemp("lanes_cli")
    mg = synth.make_metagenome(20000, 150, (("rplB", 120), ("nirK", 150), ("nifH", 100)), seed=17, reads_per_genome=1000)
    synth.write_lib_bin(mg.reads, str(d / "reads.lib"))
    gl = synth.write_gene_models(mg.genes, str(d / "models"))
    run = lambda cmd: subprocess.run(cmd, check=True, capture_output=True, timeout=CLI_LIMIT_S)
    run([BIN, "buildgraph", "-k", "44", "-m", "1", "--host_mem", "4000000000", "--mem_flag", "1", "--gpu_mem", "0", "--num_cpu_threads", "4",
         "--num_output_threads", "1", "--read_lib_file", str(d / "reads.lib"), "--output_prefix", str(d / "44")])
    for line in open(gl):
        gene, _, _, faa = line.split()
        seeds = run([BIN, "findstart", faa, str(d / "reads.lib.bin"), "45", "4"]).stdout
        assert seeds.count(b"\n") > 100, gene
        (d / f"44_{gene}_starting_kmers.txt").write_bytes(seeds)
    one = d / "gene_list_one.txt"
    one.write_text(open(gl).readline())
    lists = {"three": (gl, GENES), "one": (one, GENES[:1])}
    for tag, (gene_list, genes) in lists.items():
        r = _search(d, gene_list, f"{tag}_lanes1", None)
        assert r.returncode == 0, r.stderr[-3000:]
        for g in genes:
            assert re.search(rf"\[megagta_amd\] Done {g}: ", r.stderr), r.stderr[-3000:]
    return d, lists


@pytest.mark.parametrize("which,lanes", [("three", "2"), ("one", "2"), ("three", "7")])
def test_megagta_search_with_two_lanes_writes_the_same_files(cli_inputs, which, lanes):
    """MEGAGTA_SEARCH_LANES=2 (7 is clamped to 2): the genes of the list dealt to two threads, each with a context of its own and half of the
    CUs.  Every raw_contigs file is byte for byte the one-lane run's; with one gene the second lane finds nothing to take"""
    d, lists = cli_inputs
    gene_list, genes = lists[which]
    r = _search(d, gene_list, f"{which}_lanes{lanes}", lanes)
    assert r.returncode == 0, r.stderr[-3000:]
    for g in genes:
        assert len(re.findall(rf"\[megagta_amd\] Done {g}: ", r.stderr)) == 1, r.stderr[-3000:]
        a, b = (d / f"{which}_lanes1_raw_contigs_{g}.fasta").read_bytes(), (d / f"{which}_lanes{lanes}_raw_contigs_{g}.fasta").read_bytes()
        assert a == b and a.count(b">") > 100, (g, len(a), len(b))


# ---- f. guards ---------------------------------------------------------------------------------------------------------------------------
def test_a_refused_share_leaves_the_share_as_it_was(ctx_b, meta20k, monkeypatch, capfd):
    """num < 1, den < num: MegaGtaError, and the next batch still runs with the share set before (a sixteenth: 16 workgroups of 256 CUs)"""
    from megagta_amd import api
    monkeypatch.setenv("MGTA_ASTAR_GROUP", "16")
    monkeypatch.setenv("MGTA_ASTAR_VERBOSE", "1")
    m = meta20k
    args = (m.g, m.fw, m.rv, m.kmers, m.states, 20, 0.5)
    try:
        _, st0, baseline = _run_and_count(capfd, *args, run=ctx_b)
        ctx_b.set_search_share(1, 16)
        for bad in ((0, 1), (2, 1), (1, 0), (-1, -1)):
            with pytest.raises(api.MegaGtaError):
                ctx_b.set_search_share(*bad)
        _, st, n = _run_and_count(capfd, *args, run=ctx_b)
        assert n == _expected_workgroups(baseline, _per_device(st0), 1, 16) < baseline, (n, baseline)
    finally:
        ctx_b.set_search_share(1, 1)


def test_a_null_run_context_is_refused_and_nothing_is_written(toy):
    """mgta_astar_batch_on(NULL, ...): MGTA_EINVAL, the sink is never called and the stats stay as the caller left them"""
    from megagta_amd import _lib, api
    g, fw, rv, _ = toy
    gold = _toy_gold("astar_cold.txt.gz")[:4]
    buf = "".join(r["kmer"][:45] for r in gold).encode()
    ss = (C.c_int32 * len(gold))(*[r["start_state"] for r in gold])
    calls = []
    sink = _lib.CONTIG_SINK(lambda *a: calls.append(a) or 0)
    st = _lib.AstarStats()
    C.memset(C.byref(st), 0x5A, C.sizeof(st))
    untouched = bytes(st)
    L = g.ctx._L
    rc = L.mgta_astar_batch_on(None, g.h, fw.h, rv.h, buf, C.addressof(ss), len(gold), 20, 0.5, 0, sink, None, C.byref(st))
    assert rc == -1 and not calls and bytes(st) == untouched                # MGTA_EINVAL
    assert b"bad argument" in L.mgta_last_error()
    res, st2 = api.astar_search(g, fw, rv, [r["kmer"] for r in gold], [r["start_state"] for r in gold], 20, 0.5)      # (and the graph's context searches on)
    _check_against(res, [r["kmer"] for r in gold], gold)


def test_a_run_context_on_another_device_is_refused(toy):
    import torch
    from megagta_amd import api
    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible: a context on another device cannot be made")
    g, fw, rv, _ = toy
    gold = _toy_gold("astar_cold.txt.gz")[:4]
    other = api.Context(1)
    try:
        with pytest.raises(api.MegaGtaError, match="the context and the graph live on different devices"):
            api.astar_search(g, fw, rv, [r["kmer"] for r in gold], [r["start_state"] for r in gold], 20, 0.5, run=other)
    finally:
        other.close()


if __name__ == "__main__":
    _child(sys.argv[1])
