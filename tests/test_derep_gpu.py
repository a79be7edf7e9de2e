"""De-replication (Context.derep / `megagta derep` / `megagta.py --derep`): the unique, non-contained sequences of a set.

Expected values never come from the code under test: they are Python's `==`, `in` and dict.setdefault over the strings.  Every
comparison is exact: the outputs are integers."""
import os
import subprocess
import sys

import numpy as np
import pytest

from megagta_amd import derep as dr
from megagta_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "megagta_amd", "bin", "megagta")
DRIVER = os.path.join(ROOT, "megagta_amd", "megagta.py")
AA = "acdefghiklmnpqrstvwy"


def make_input(seed=7):
    """553 sequences over the 20 amino-acid letters: parents, their pieces (around the anchor length and the 16-byte lane width, at the
    first, the last and an inner position), near-pieces with one letter changed, exact copies, chimeras, low-complexity runs that put
    many windows of one sequence into one list, the empty sequence; permuted"""
    rng = np.random.default_rng(seed)

    def rand(n):
        return "".join(AA[c] for c in rng.integers(0, 20, n))

    parents = [rand(300) for _ in range(6)]
    seqs = list(parents)
    for _ in range(400):
        p = parents[int(rng.integers(0, 6))]
        n = int(rng.integers(1, 301))
        a = int(rng.integers(0, 300 - n + 1))
        seqs.append(p[a:a + n])
    for j, n in enumerate((15, 16, 17, 31, 32, 33)):
        p = parents[j]
        a = int(rng.integers(1, 300 - n))
        seqs += [p[:n], p[300 - n:], p[a:a + n]]
    for j in range(60):
        s = seqs[6 + int(rng.integers(0, 400))]
        at = (0, len(s) - 1, len(s) // 2)[j % 3]
        c = AA[(AA.index(s[at]) + 1 + int(rng.integers(0, 19))) % 20]     # always another letter
        seqs.append(s[:at] + c + s[at + 1:])
    for _ in range(60):
        seqs.append(seqs[int(rng.integers(0, len(seqs)))])
    A, B, D = parents[0], parents[1], parents[3]
    seqs += [A[:150] + B[150:], D[:100] + D[120:]]
    seqs += ["a" * 40, "a" * 39, "a" * 16, "ab" * 30, "ab" * 29 + "a", "ba" * 10, ""]
    return [seqs[i] for i in rng.permutation(len(seqs))]


def brute_force(seqs):
    """the rule, literally"""
    first, count = {}, {}
    for i, s in enumerate(seqs):
        first.setdefault(s, i)
        count[s] = count.get(s, 0) + 1
    distinct = list(first)
    status, rep, copies = [], [], []
    for i, s in enumerate(seqs):
        if first[s] != i:
            status.append(1), rep.append(first[s]), copies.append(0)
            continue
        c = any(len(t) > len(s) and s in t for t in distinct)
        status.append(2 if c else 0), rep.append(-1 if c else i), copies.append(count[s])
    return np.array(status, dtype=np.uint8), np.array(rep, dtype=np.int64), np.array(copies, dtype=np.uint32)


def assert_is(res, want):
    for name, w in zip(("status", "rep", "copies"), want):
        assert res[name].dtype == w.dtype and np.array_equal(res[name], w), (name, np.flatnonzero(res[name] != w)[:10])


def assert_stats_fit(st, seqs, want):
    status = want[0]
    assert st["n_seqs"] == len(seqs) and st["n_letters"] == sum(len(s) for s in seqs)
    assert st["n_duplicates"] == int((status == 1).sum()) and st["n_contained"] == int((status == 2).sum()) and st["n_kept"] == int((status == 0).sum())
    assert st["n_first"] == st["n_kept"] + st["n_contained"] == len(set(seqs))
    firsts = [s for s in set(seqs) if s]
    a = min([16] + [len(s) for s in firsts]) if firsts else 0
    assert st["anchor_len"] == a
    assert st["n_windows"] == (sum(len(s) - a + 1 for s in firsts) if len(set(seqs)) > 1 else 0)


def stable(st):
    return {n: v for n, v in st.items() if not n.startswith("ms_") and n != "n_compares"}


@pytest.fixture(scope="module")
def ctx():
    from megagta_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def case():
    seqs = make_input()
    return dict(seqs=seqs, want=brute_force(seqs))


# ---- 1. brute force ----------------------------------------------------------------------------------------------------------------
def test_equals_brute_force(ctx, case):
    seqs, want = case["seqs"], case["want"]
    assert len(seqs) == 553
    for cls in (0, 1, 2):
        assert (want[0] == cls).any()
    res = ctx.derep(seqs)
    assert_is(res, want)
    assert_stats_fit(res["stats"], seqs, want)
    assert res["stats"]["anchor_len"] == 1
    long_only = [s for s in seqs if len(s) >= 16]
    assert 0 < len(long_only) < len(seqs)
    want16 = brute_force(long_only)
    res16 = ctx.derep(long_only)
    assert_is(res16, want16)
    assert_stats_fit(res16["stats"], long_only, want16)
    assert res16["stats"]["anchor_len"] == 16
    assert_is(ctx.derep([s.encode() for s in seqs]), want)               # bytes in, the same out


# ---- 2. collisions -----------------------------------------------------------------------------------------------------------------
def test_hash_collisions_change_no_answer(ctx, case):
    seqs, want = case["seqs"], case["want"]
    out = {}
    try:
        for bits in (4, 1, 64):
            ctx.set_derep_hash_bits(bits)
            out[bits] = ctx.derep(seqs)
    finally:
        ctx.set_derep_hash_bits(64)
    for bits, res in out.items():
        assert_is(res, want)
        assert stable(res["stats"]) == stable(out[64]["stats"]), bits
        for name in ("status", "rep", "copies"):
            assert res[name].tobytes() == out[64][name].tobytes(), (bits, name)
    print("n_compares at 4, 1, 64 bits:", [out[b]["stats"]["n_compares"] for b in (4, 1, 64)])
    assert out[4]["stats"]["n_compares"] > out[64]["stats"]["n_compares"]   # the switch acts


# ---- 3. order and determinism ------------------------------------------------------------------------------------------------------
def test_two_calls_and_two_orders(ctx, case):
    seqs = case["seqs"]
    a, b = ctx.derep(seqs), ctx.derep(seqs)
    for name in ("status", "rep", "copies"):
        assert a[name].tobytes() == b[name].tobytes(), name
    assert stable(a["stats"]) == stable(b["stats"])
    perm = np.random.default_rng(8).permutation(len(seqs))
    other = [seqs[i] for i in perm]
    c = ctx.derep(other)
    assert_is(c, brute_force(other))

    def kept_and_copies(ss, res):
        return ({s for s, st in zip(ss, res["status"]) if st == 0}, {s: int(n) for s, st, n in zip(ss, res["status"], res["copies"]) if st != 1})

    assert kept_and_copies(seqs, a) == kept_and_copies(other, c)


# ---- 4. edges ----------------------------------------------------------------------------------------------------------------------
def test_edges(ctx):
    res = ctx.derep([])
    assert res["status"].size == 0 and res["rep"].size == 0 and res["copies"].size == 0 and all(v == 0 for v in res["stats"].values())
    rng = np.random.default_rng(21)
    big = "".join(AA[c] for c in rng.integers(0, 20, 5000))               # more windows than a 256-thread workgroup holds
    piece = big[2500:2517]
    near = piece[:8] + ("a" if piece[8] != "a" else "c") + piece[9:]
    cases = {
        "one": ["mkvlaagh"],
        "identical": ["mkvlaagh"] * 70,
        "all empty": [""] * 9,
        "empty and one": ["", "m", ""],
        "long and its piece": [big, piece, near, big[:16], big[-16:], big[1:], big],
        "zero bytes are letters": [b"ab\0", b"ab", b"ab\0\0", b"\0"],
    }
    for name, seqs in cases.items():
        want = brute_force(seqs)
        res = ctx.derep(seqs)
        assert_is(res, want)
        assert_stats_fit(res["stats"], seqs, want)
    res = ctx.derep(cases["all empty"])
    assert res["status"].tolist() == [0] + [1] * 8 and res["copies"][0] == 9 and res["stats"]["anchor_len"] == 0
    res = ctx.derep(cases["long and its piece"])
    assert res["status"].tolist() == [0, 2, 0, 2, 2, 2, 1]


# ---- 5. guards ---------------------------------------------------------------------------------------------------------------------
def test_guards(ctx):
    L = ctx._L
    off = np.array([0, 4, 8], dtype=np.uint64)
    status, rep, copies = np.full(2, 77, dtype=np.uint8), np.full(2, 77, dtype=np.int64), np.full(2, 77, dtype=np.uint32)
    args = (b"mkvlmkvl", off.ctypes.data, 2)
    outs = (status.ctypes.data, rep.ctypes.data, copies.ctypes.data)
    assert L.mgta_seqs_derep(None, *args, *outs, None) == -1 and b"ctx" in L.mgta_last_error()
    for i, name in enumerate((b"status", b"rep", b"copies")):
        o = list(outs)
        o[i] = None
        assert L.mgta_seqs_derep(ctx.h, *args, *o, None) == -1 and name in L.mgta_last_error()
    assert L.mgta_seqs_derep(ctx.h, b"mkvlmkvl", None, 2, *outs, None) == -1 and b"offsets" in L.mgta_last_error()
    assert L.mgta_seqs_derep(ctx.h, b"mkvlmkvl", off.ctypes.data, -1, *outs, None) == -1 and b"n = -1" in L.mgta_last_error()
    down = np.array([0, 8, 4], dtype=np.uint64)
    assert L.mgta_seqs_derep(ctx.h, b"mkvlmkvl", down.ctypes.data, 2, *outs, None) == -1 and b"offsets must ascend" in L.mgta_last_error()
    for bits in (0, 65):
        assert L.mgta_ctx_set_derep_hash_bits(ctx.h, bits) == -1 and b"bits" in L.mgta_last_error()
    assert L.mgta_ctx_set_derep_hash_bits(None, 8) == -1 and b"ctx" in L.mgta_last_error()
    assert (status == 77).all() and (rep == 77).all() and (copies == 77).all()   # nothing was written by the refused calls
    assert L.mgta_seqs_derep(ctx.h, *args, *outs, None) == 0            # the same arguments with everything in place: a valid call
    assert status.tolist() == [0, 1] and rep.tolist() == [0, 0] and copies.tolist() == [2, 0]
    assert L.mgta_seqs_derep(ctx.h, None, None, 0, None, None, None, None) == 0


# ---- 6. process boundary -----------------------------------------------------------------------------------------------------------
def test_one_shot_and_worker_write_the_same_files(ctx, case, tmp_path):
    assert os.path.exists(BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    sets = (case["seqs"], [s for s in case["seqs"] if len(s) >= 16][:200])
    inputs = []
    for i, seqs in enumerate(sets):
        headers = [f"c{j} len={len(s)}" if j % 3 else f"c{j}" for j, s in enumerate(seqs)]
        nucl = ["ACGT"[j % 4] * (3 * len(s)) for j, s in enumerate(seqs)]
        prot, nuc = str(tmp_path / f"p{i}.fa"), str(tmp_path / f"n{i}.fa")
        open(prot, "w").write("".join(f">{h}\n{s}\n" for h, s in zip(headers, seqs)))
        open(nuc, "w").write("".join(f">c{j} x\n{s}\n" for j, s in enumerate(nucl)))
        inputs.append((headers, nucl, prot, nuc))
    for i, (_, _, prot, nuc) in enumerate(inputs):
        subprocess.run([BIN, "derep", prot, str(tmp_path / f"one{i}"), nuc, str(tmp_path / f"one{i}n")], check=True, capture_output=True, timeout=120)
    req = "".join(f"derep\t{prot}\t{tmp_path}/w{i}\t{nuc}\t{tmp_path}/w{i}n\n" for i, (_, _, prot, nuc) in enumerate(inputs)) + "quit\n"
    r = subprocess.run([BIN, "serve"], input=req, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["DONE", "0", "DONE", "0"], r.stderr[-2000:]
    for i, seqs in enumerate(sets):
        headers, nucl = inputs[i][:2]
        res = ctx.derep(seqs)
        names = [dr.record_name(h) for h in headers]
        want = {"_rmdup.fasta": dr.rmdup_fasta_text(headers, seqs, res["status"]),
                "_rmdup_map.txt": dr.map_text(names, res["status"], res["rep"], res["copies"]),
                "n_rmdup.fasta": dr.rmdup_fasta_text([f"c{j} x" for j in range(len(seqs))], nucl, res["status"])}
        for tail, text in want.items():
            assert open(f"{tmp_path}/one{i}{tail}").read() == open(f"{tmp_path}/w{i}{tail}").read() == text and len(text) > 0, (i, tail)
        back = dr.read_map(f"{tmp_path}/one{i}_rmdup_map.txt")
        assert np.array_equal(back["status"], res["status"]) and np.array_equal(back["rep"], res["rep"]) and np.array_equal(back["copies"], res["copies"])
    # without the nucleotide pair: the two protein files alone
    subprocess.run([BIN, "derep", inputs[1][2], str(tmp_path / "solo")], check=True, capture_output=True, timeout=120)
    assert open(tmp_path / "solo_rmdup.fasta").read() == open(tmp_path / "one1_rmdup.fasta").read()
    assert open(tmp_path / "solo_rmdup_map.txt").read() == open(tmp_path / "one1_rmdup_map.txt").read()
    # a nucleotide file with one name changed, or one record short: the step fails and leaves nothing
    text = open(inputs[1][3]).read()
    for j, bad in enumerate((text.replace(">c7 x\n", ">c7b x\n"), text[:text.rindex(">")])):
        assert bad != text
        open(tmp_path / "bad.fa", "w").write(bad)
        r = subprocess.run([BIN, "derep", inputs[1][2], str(tmp_path / f"bad{j}"), str(tmp_path / "bad.fa"), str(tmp_path / f"bad{j}n")], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode != 0 and "derep" in r.stderr
        assert [f for f in os.listdir(tmp_path) if f.startswith(f"bad{j}")] == []


# ---- 7. driver end to end ----------------------------------------------------------------------------------------------------------
def _tree(root):
    out = {}
    for dp, _, fs in os.walk(root):
        for f in fs:
            p = os.path.join(dp, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def _records(text):
    """[(header line, sequence)] of a FASTA text with one-line sequences"""
    lines = text.splitlines()
    assert len(lines) % 2 == 0 and all(h.startswith(">") for h in lines[0::2])
    return [(h[1:], s) for h, s in zip(lines[0::2], lines[1::2])]


_CODON = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF"


def translate(nucl):
    """`megagta translate`: frame 0, the standard code, lower case, x for a codon with a letter outside ACGT"""
    code = {"A": 0, "C": 1, "G": 2, "T": 3, "U": 3}
    out = []
    for i in range(0, len(nucl) - 2, 3):
        c = [code.get(x, -1) for x in nucl[i:i + 3].upper()]
        out.append("x" if min(c) < 0 else _CODON[16 * c[0] + 4 * c[1] + c[2]].lower())
    return "".join(out)


def test_driver_derep_end_to_end(golden_dir, tmp_path):
    assert os.path.exists(BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    mg = synth.make_metagenome(6000, 150, (("rplB", 100),), seed=11, reads_per_genome=1000)    # the sample of the match-reads test
    synth.write_fasta(mg.reads, str(tmp_path / "reads.fa"))
    toy = os.path.join(golden_dir, "toy")
    (tmp_path / "gene_list.txt").write_text(f"rplB {toy}/for_enone.hmm {toy}/rev_enone.hmm {toy}/ref_aligned.faa\n")
    base = [sys.executable, DRIVER, "-r", str(tmp_path / "reads.fa"), "-g", str(tmp_path / "gene_list.txt"), "-k", "45", "-t", "4", "--min-contig-len", "150"]
    runs = {"dr": ["--derep"], "all_1p": ["--coverage", "--match-reads", "--derep", "--one-process-per-step"]}
    trees = {}
    for name, extra in runs.items():
        out = tmp_path / name
        r = subprocess.run(base + ["-o", str(out)] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr + open(out / "log").read()[-2000:]
        trees[name] = _tree(str(out))
    d = "contigs/rplB/"
    new = [d + "prot_merged_rmdup.fasta", d + "prot_merged_rmdup_map.txt", d + "nucl_merged_rmdup.fasta"]
    for f in new:
        assert trees["dr"][f] == trees["all_1p"][f] and len(trees["dr"][f]) > 0, f
    volatile = {"log", "opts.txt", "tmp/cp.txt"}
    assert set(trees["all_1p"]) - set(trees["dr"]) == {d + "nucl_merged_coverage.txt", d + "nucl_merged_abundance.txt", d + "nucl_merged_match_reads.fa"}
    assert set(trees["dr"]) <= set(trees["all_1p"])
    for f in (set(trees["dr"]) & set(trees["all_1p"])) - volatile:
        assert trees["dr"][f] == trees["all_1p"][f], f
    # against brute force over prot_merged.fasta
    prot = _records(trees["dr"][d + "prot_merged.fasta"].decode())
    nucl = _records(trees["dr"][d + "nucl_merged.fasta"].decode())
    status, rep, copies = brute_force([s for _, s in prot])
    assert (status == 0).any() and (status != 0).any()
    kept = [r for r, st in zip(prot, status) if st == 0]
    assert _records(trees["dr"][new[0]].decode()) == kept
    names = [dr.record_name(h) for h, _ in prot]
    assert trees["dr"][new[1]].decode() == dr.map_text(names, status, rep, copies)
    nucl_kept = _records(trees["dr"][new[2]].decode())
    assert nucl_kept == [r for r, st in zip(nucl, status) if st == 0]
    assert [dr.record_name(h) for h, _ in nucl_kept] == [dr.record_name(h) for h, _ in kept]
    assert [translate(s) for _, s in nucl_kept] == [s for _, s in kept]
    # one checkpoint for the flag's step (one gene), behind every checkpoint of the steps before it: buildlib, buildgraph, findstart, then
    # filterbylen + translate inside the search step and the search's own = 6 before the flag's; coverage and match-reads add one each
    cp_dr = trees["dr"]["tmp/cp.txt"].decode().splitlines()
    cp_all = trees["all_1p"]["tmp/cp.txt"].decode().splitlines()
    assert cp_dr == [f"{i}\tdone" for i in range(6 + 1)]
    assert cp_all == [f"{i}\tdone" for i in range(6 + 3)]
    # --continue on the finished run does nothing and succeeds
    out = tmp_path / "dr"
    r = subprocess.run([sys.executable, DRIVER, "--continue", "-o", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0
    after = _tree(str(out))
    for f in new:
        assert after[f] == trees["dr"][f], f
    assert after["log"].count(b"De-replicating") == trees["dr"]["log"].count(b"De-replicating") == 1    # the step did not run again
