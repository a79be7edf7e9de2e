"""Position-specific profile HMMs for the tests (test code only; megagta_amd.synth.hmm_text and its goldens stay as they are).

synth.hmm_text writes one transition row for every node, m->i == m->d, i->m == i->i and two-valued match columns: max_match is one
constant, the heuristic is linear in the column, and a kernel that reads a table one node off, or swaps two of those transitions, or
two non-consensus letters, computes the same numbers.  The models written here are what HMMER builds from a real family, in every one
of those tables:

  * COMPO is a Dirichlet draw;
  * every node has its own match column: the mass on the consensus letter runs from 0.15 (delete-friendly nodes: a nearly flat column)
    to 0.9, the other 19 letters are all distinct;
  * every node has its own seven transitions, pairwise distinct, different from its neighbours';
  * a handful of nodes are insert-friendly (high m->i and i->i), a handful of stretches delete-friendly (high m->d and d->d over flat
    columns): there the A* heuristic continues through D, and best paths go through I and D;
  * with stars=True a few entries are `*`: one match emission of a non-consensus letter, m->d, or m->i -- never two in one row;
  * node 0 and node M are synth.hmm_text's (what the three parsers require); insert emission lines too (the reference forces 0).

Everything is a function of the arguments (numpy's default_rng(seed)); the numbers are printed with five decimals, as HMMER prints."""
from __future__ import annotations

import gzip
import hashlib
import json
import os

import numpy as np

from megagta_amd.synth import AA_ORDER

MM, MI, MD, IM, II, DM, DD = range(7)
HEADER = ["HMMER3/b [synthetic | tests.rich_models]", None, None, "ALPH  amino", "RF    no", "CS    no", "MAP   yes", "STATS LOCAL MSV      -9.0000  0.70000",
          "HMM          " + "        ".join(AA_ORDER), "            m->m     m->i     m->d     i->m     i->i     d->m     d->d"]


def _nl(p: float) -> str:
    return "%.5f" % (-np.log(p))


def rich_layout(M: int, seed: int, n_insert: int | None = None, n_delete: int | None = None, **_):
    """-> (insert-friendly nodes, delete-friendly stretches [(first, last)]), 1-based columns, apart from each other and from the ends.
    An insert-friendly node j holds its residues between columns j and j + 1; a delete-friendly stretch is a run of two or three
    columns that best paths leave out."""
    rng = np.random.default_rng([seed, M, 17])
    n_insert = max(0, (M - 6) // 20) if n_insert is None else n_insert
    n_delete = max(0, (M - 6) // 25) if n_delete is None else n_delete
    slots = list(range(3, M - 5, 6))                                      # a slot owns the columns [s, s + 5]
    pick = [slots[i] for i in sorted(rng.permutation(len(slots))[:n_insert + n_delete])]
    kinds = rng.permutation([0] * n_insert + [1] * n_delete)[:len(pick)]
    ins, dels = [], []
    for s, kind in zip(pick, kinds):
        if kind == 0:
            ins.append(s + int(rng.integers(0, 3)))
        else:
            a = s + int(rng.integers(0, 2))
            dels.append((a, a + int(rng.integers(1, 3))))
    return ins, dels


def rich_hmm_text(name: str, consensus: str, seed: int, stars: bool = False, p_cons=(0.35, 0.9), **shape) -> str:
    """HMMER3 text of a position-specific model around `consensus` (see the module's text); shape: stars, p_cons = the range of the
    consensus letter's mass at the ordinary nodes, n_insert / n_delete = how many friendly nodes / stretches (rich_layout)"""
    M = len(consensus)
    rng = np.random.default_rng([seed, M, 29])
    ins, dels = rich_layout(M, seed, **shape)
    flat = {j for a, b in dels for j in range(a, b + 1)}
    del_rows = {j for a, b in dels for j in range(a - 1, b + 1)}           # row j holds the transitions into column j + 1
    out = list(HEADER)
    out[1], out[2] = f"NAME  {name}", f"LENG  {M}"
    compo = rng.dirichlet(np.ones(20) * 3)
    compo = np.maximum(compo, 0.012)
    compo /= compo.sum()
    out.append("  COMPO   " + "  ".join(_nl(p) for p in compo))
    uni = "  ".join([_nl(0.05)] * 20)
    out.append("          " + uni)
    out.append("          " + "  ".join([_nl(0.98), _nl(0.01), _nl(0.01), _nl(0.5), _nl(0.5), _nl(1.0), "*"]))
    prev = None
    for j, a in enumerate(consensus, start=1):
        c = AA_ORDER.index(a)
        while True:                                                       # the match column: 20 distinct numbers as printed
            if j in flat:
                pc = 0.15
                rest = rng.dirichlet(np.delete(compo, c) * 150) * (1 - pc)  # close to the background: the column says little
            else:
                pc = float(rng.uniform(*p_cons))
                rest = rng.dirichlet(np.ones(19)) * (1 - pc)
            rest = np.maximum(rest, 1e-6)
            em = [_nl(p) for p in np.insert(rest, c, pc)]
            if len(set(em)) == 20 and rest.max() < pc:
                break
        if stars and j % 7 == 3:
            em[(c + 1 + int(rng.integers(0, 19))) % 20] = "*"             # never the consensus letter
        out.append(f"{j:7d}   " + "  ".join(em) + f"  {j:6d} - -")
        out.append("          " + uni)
        if j == M:
            out.append("          " + "  ".join([_nl(0.99), _nl(0.01), "*", _nl(0.5), _nl(0.5), _nl(1.0), "*"]))
            break
        while True:                                                       # the seven transitions: distinct as printed, not the row before
            if j in del_rows:
                mi, md, ii, dd = rng.uniform(0.004, 0.01), rng.uniform(0.80, 0.88), rng.uniform(0.2, 0.6), rng.uniform(0.6, 0.8)
            elif j in ins:
                mi, md, ii, dd = rng.uniform(0.3, 0.45), rng.uniform(0.004, 0.03), rng.uniform(0.6, 0.8), rng.uniform(0.15, 0.5)
            else:
                mi, md, ii, dd = rng.uniform(0.004, 0.03), rng.uniform(0.004, 0.03), rng.uniform(0.2, 0.6), rng.uniform(0.15, 0.5)
            tr = [_nl(1 - mi - md), _nl(mi), _nl(md), _nl(1 - ii), _nl(ii), _nl(1 - dd), _nl(dd)]
            if len(set(tr)) == 7 and (prev is None or all(x != y for x, y in zip(tr, prev))):
                break
        prev = list(tr)
        if stars and j not in del_rows and j not in ins:
            if j % 11 == 4:
                tr[MD] = "*"                                              # no way into D here
            elif j % 13 == 6:
                tr[MI] = "*"                                              # no way into I here
        out.append("          " + "  ".join(tr))
    out.append("//")
    return "\n".join(out) + "\n"


def rich_gene_models(gene, outdir: str, seed: int, **shape) -> str:
    """<outdir>/<gene.name>/for_enone.hmm around the gene's consensus, rev_enone.hmm around the reversed consensus with draws of its
    own, ref_aligned.faa: what synth.write_gene_models writes, so synth.make_metagenome's reads and findstart's seeds work unchanged
    -> the gene's directory"""
    d = os.path.join(outdir, gene.name)
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "for_enone.hmm"), "w") as f:
        f.write(rich_hmm_text(gene.name, gene.consensus, seed, **shape))
    with open(os.path.join(d, "rev_enone.hmm"), "w") as f:
        f.write(rich_hmm_text(gene.name + "_rev", gene.consensus[::-1], seed + 1000, **shape))
    with open(os.path.join(d, "ref_aligned.faa"), "w") as f:
        f.write(f">{gene.name}_consensus\n{gene.consensus}\n")
    return d


# ---- the deliberately wrong models of the sensitivity check: each is the mistake of a kernel written into the model's text, so that the
# yardstick alone, run on it, shows whether the test inputs can see that mistake
def _rows(text: str):
    """-> (lines, {node: index of its match line}); the transitions of node j are lines[at[j] + 2], of node 0 lines[at[1] - 1]"""
    lines = text.split("\n")
    at = {}
    for n, line in enumerate(lines):
        t = line.split()
        if len(t) >= 21 and t[0].isdigit():
            at[int(t[0])] = n
    return lines, at


WRONG = ("transitions_up", "match_up", "mi_md", "im_ii", "dm_dd", "letters")


def wrong_model_text(text: str, kind: str) -> str:
    """the model with one mistake: the transition rows (or the match rows) of the nodes 1 .. M - 1 moved one node up (node j takes
    node j + 1's, node M - 1 takes node 1's), two transition columns swapped at every node 1 .. M - 1, or the match columns of the
    letters D and K swapped at every node whose consensus letter is neither"""
    lines, at = _rows(text)
    M = len(at)
    inner = list(range(1, M))
    if kind == "transitions_up":
        rows = [lines[at[j] + 2] for j in inner]
        for j, row in zip(inner, rows[1:] + rows[:1]):
            lines[at[j] + 2] = row
    elif kind == "match_up":
        rows = [lines[at[j]].split()[1:21] for j in inner]
        for j, row in zip(inner, rows[1:] + rows[:1]):
            t = lines[at[j]].split()
            lines[at[j]] = f"{j:7d}   " + "  ".join(row + t[21:])
    elif kind in ("mi_md", "im_ii", "dm_dd"):
        x, y = {"mi_md": (MI, MD), "im_ii": (IM, II), "dm_dd": (DM, DD)}[kind]
        for j in inner:
            t = lines[at[j] + 2].split()
            t[x], t[y] = t[y], t[x]
            lines[at[j] + 2] = "          " + "  ".join(t)
    elif kind == "letters":
        x, y = 1 + AA_ORDER.index("D"), 1 + AA_ORDER.index("K")
        for j in range(1, M + 1):
            t = lines[at[j]].split()
            if min(range(1, 21), key=lambda i: float("inf") if t[i] == "*" else float(t[i])) in (x, y):
                continue                                                  # the consensus letter's column stays: a two-valued model would see that
            t[x], t[y] = t[y], t[x]
            lines[at[j]] = f"{j:7d}   " + "  ".join(t[1:])
    else:
        raise ValueError(kind)
    return "\n".join(lines)


# ---- tests/golden/richm: the reference's answers on these models (make_golden_richm.py).  Reads and seeds regenerate from their seeds.
RICHM_CASES = {"r75": dict(M=75, n_reads=4000, seed=71, model_seed=5, prune=20, stars=False, n_seeds=40),
               "r130": dict(M=130, n_reads=4000, seed=72, model_seed=6, prune=0, stars=True, n_seeds=40),
               "r600": dict(M=600, n_reads=2400, seed=73, model_seed=7, prune=20, stars=False, n_seeds=32),
               # (600 columns still fit the LDS beside the heap tops of ONE search per wavefront: the 64-lane kernel reads its tables from
               # device memory from about 630 columns on)
               "r700": dict(M=700, n_reads=2400, seed=74, model_seed=8, prune=20, stars=False, n_seeds=8)}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "richm")


def tables_md5(t) -> str:
    """md5 over the bits of the tables in helpers.parse_probe_hmm's layout (M, A, alpha, then msc of the nodes 1 .. M, tsc, maxm and h of
    the nodes 0 .. M as little-endian doubles): what stands for a 600-column model's tables, which would be a quarter of a megabyte"""
    M = int(t["M"])
    h = hashlib.md5(np.array([M, int(t["A"])] + [int(x) for x in t["alpha"]], dtype="<i8").tobytes())
    for k in range(1, M + 1):
        h.update(np.asarray(t["msc"][k], dtype="<f8").tobytes())
    for k in range(M + 1):
        h.update(np.asarray(t["tsc"][k], dtype="<f8").tobytes() + np.asarray([t["maxm"][k]], dtype="<f8").tobytes() + np.asarray(t["h"][k], dtype="<f8").tobytes())
    return h.hexdigest()


def richm_inputs(case: str, outdir: str):
    """the seeded inputs of one case -> (metagenome, gene dir with the two models and ref_aligned.faa written)"""
    from megagta_amd import synth
    c = RICHM_CASES[case]
    mg = synth.make_metagenome(c["n_reads"], 150, ((case, c["M"]),), seed=c["seed"], reads_per_genome=600, genome_len=6000)
    return mg, rich_gene_models(mg.genes[0], os.path.join(outdir, "genes"), c["model_seed"], stars=c["stars"])


def richm_case(case: str, outdir: str):
    """-> (packed reads, start_idx, gene dir, {"cold": goldens, "warm": goldens where stored}); the regenerated inputs are checked
    against the md5s stored with the goldens, and r75 / r130's models against the committed texts"""
    from megagta_amd import synth
    from tests import helpers as H
    meta = json.load(open(os.path.join(GOLDEN, "cases.json")))[case]
    mg, gdir = richm_inputs(case, outdir)
    for tag, name in (("for", "for_enone.hmm"), ("rev", "rev_enone.hmm")):
        data = open(os.path.join(gdir, name), "rb").read()
        assert hashlib.md5(data).hexdigest() == meta["md5"][tag], f"{case}: regenerated {name} differs from the generator's"
        stored = os.path.join(GOLDEN, f"{case}_{name}")
        if os.path.exists(stored):
            assert open(stored, "rb").read() == data, f"{case}: {name} differs from the committed text"
    synth.write_lib_bin(mg.reads, os.path.join(outdir, "reads.lib"))
    assert hashlib.md5(open(os.path.join(outdir, "reads.lib.bin"), "rb").read()).hexdigest() == meta["md5"]["reads"], f"{case}: regenerated reads differ"
    packed, start = synth.pack_reads_for_build(mg.reads)
    gold = {}
    for mode in ("cold", "warm"):
        p = os.path.join(GOLDEN, f"{case}_astar_{mode}.txt.gz")
        if os.path.exists(p):
            with gzip.open(p, "rt") as f:
                gold[mode] = H.parse_probe_astar(f.read().splitlines())
    return packed, start, gdir, gold


# ---- the protein stages (align, posterior, recruit): rich models at the strip and lane edges, and sequences that make best paths go
# through I and D where the model invites them.  The host tests (can the yardsticks see a mistake on these inputs?) and the GPU tests
# (does the device agree with the yardsticks on them?) use the same ones.
PROTEIN_MS = (1, 2, 63, 64, 65, 129)
LENGTHS = (1, 2, 63, 64, 65, 130)
AA = AA_ORDER.lower()


def rich_protein_model(M: int):
    """-> (consensus, model text, seed) of the rich model of M columns; `*` entries in the odd widths above 2"""
    from tests.test_align_gpu import protein
    seed = 500 + M
    cons = protein(np.random.default_rng(seed), M)
    return cons, rich_hmm_text(f"rich{M}", cons, seed, stars=(M % 2 == 1 and M > 2)), seed


def emission_sample(hm, rng) -> str:
    """one letter per column drawn from the column's own match emissions (p = exp(msc) * compo)"""
    letters = {int(hm.alpha[ord(c)]): c for c in AA}
    out = []
    for j in range(1, hm.M + 1):
        p = np.exp(hm.msc[j]) * hm.compo
        out.append(letters[int(rng.choice(hm.A, p=p / p.sum()))])
    return "".join(out)


def rich_sequences(hm, cons: str, seed: int, lengths=LENGTHS):
    """[(kind, sequence)]: for every length a piece of the consensus (repeated where it is longer than the model) and letters at random;
    a sample of the model's own emissions at the lengths that fit; the consensus with a run of residues behind every insert-friendly
    node; the consensus without the columns of every delete-friendly stretch.  The gapped ones have a length of `lengths` too where the
    model is long enough."""
    M = hm.M
    rng = np.random.default_rng([seed, 3])
    ins, dels = rich_layout(M, seed)
    low = cons.lower()
    rand = lambda n: "".join(AA[c] for c in rng.integers(0, 20, n))        # noqa: E731
    out = []
    for L in lengths:
        a = int(rng.integers(0, max(1, M - L + 1))) if L <= M else int(rng.integers(0, M))
        out.append(("piece", (low * (L // M + 2))[a:a + L]))
        out.append(("random", rand(L)))
        s = emission_sample(hm, rng)
        if L <= M:
            a = int(rng.integers(0, M - L + 1))
            out.append(("emitted", s[a:a + L]))
    long_ones = [L for L in lengths if L > 20]
    for n, j in enumerate(ins):
        L, run = long_ones[n % len(long_ones)], 2 + n % 3
        W = min(L - run, M)
        a = int(np.clip(j - W // 2, max(0, j + 1 - W), min(j - 1, M - W)))  # the window holds the columns j and j + 1
        out.append(("inserted", low[a:j] + rand(run) + low[j:a + W]))
    for n, (d0, d1) in enumerate(dels):
        L = long_ones[(n + 1) % len(long_ones)]
        W = min(L + d1 - d0 + 1, M)
        a = int(np.clip(d0 - W // 2, max(0, d1 + 1 - W), min(d0 - 2, M - W)))  # the window holds the columns d0 - 1 and d1 + 1
        out.append(("deleted", low[a:d0 - 1] + low[d1:a + W]))
    return out


def rich_reads(seqs, seed: int):
    """one read per sequence that codes for it, in frame (index mod 6): frames 0 .. 2 behind that many bases, frames 3 .. 5 on the
    other strand; up to two bases behind the last codon"""
    from tests.test_recruit_gpu import coding, revcomp
    rng = np.random.default_rng([seed, 4])
    reads = []
    for n, s in enumerate(seqs):
        f = n % 6
        r = np.concatenate([rng.integers(0, 4, f % 3, dtype=np.uint8), coding(rng, s.upper()), rng.integers(0, 4, int(rng.integers(0, 3)), dtype=np.uint8)])
        reads.append(revcomp(r) if f >= 3 else r)
    return reads
