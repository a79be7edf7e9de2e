#!/usr/bin/env python3
"""The rate of mgta_reads_pileup next to mgta_contig_sample_coverage with one library: the same graph, reads and contigs, one process.

python scripts/pileup_rate.py [--contigs 20000] [--depth 2] [--foreign 0.2] [--k 20] [--repeat 3] [--out profiles/pileup/run.json]

The contigs are nucleotide pieces of 360 to 540 letters (120 to 180 residues) of variants of one random gene of 900 letters, in the
shape of scripts/nearest_rate.py: a variant has one letter in ten substituted and a few insertions and deletions of 1 to 5 letters.
The reads are 100 letters drawn from the contigs, `depth` times the contigs' letters in all, every second one reverse-complemented, with
1 % substitutions; a share `foreign` of the reads is random.  The graph is the `-m 1` graph of these reads.  A second input has only
random reads: no read matches, both scans do the same walk and nothing else.  Per input one JSON line: reads per second of the pileup
(ms_total, HIP events of the library), its ms_* per phase, candidates and verified candidates per placed read, the per-library scan's
ms_total and the ratio of the two.  The first call of each is a warm-up; the best of `repeat` further calls is reported next to all."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from megagta_amd import api, readlib  # noqa: E402

DNA = np.frombuffer(b"ACGT", dtype=np.uint8)


def variant(rng, gene: np.ndarray) -> np.ndarray:
    s = gene.copy()
    hit = rng.random(s.size) < 0.1
    s[hit] = rng.integers(0, 4, int(hit.sum()))
    for _ in range(int(rng.integers(0, 4))):
        at, n = int(rng.integers(5, s.size - 10)), int(rng.integers(1, 6))
        s = np.concatenate([s[:at], s[at + n:]]) if rng.random() < 0.5 else np.concatenate([s[:at], rng.integers(0, 4, n).astype(np.uint8), s[at:]])
    return s


def make_reads(rng, contigs, depth: float, foreign: float, only_foreign: bool):
    letters = sum(c.size for c in contigs)
    n = max(1, int(letters * depth / 100))
    reads = []
    for r in range(n):
        if only_foreign or rng.random() < foreign:
            reads.append(rng.integers(0, 4, 100).astype(np.uint8))
            continue
        c = contigs[int(rng.integers(0, len(contigs)))]
        at = int(rng.integers(0, c.size - 100 + 1))
        s = c[at:at + 100].copy()
        hit = rng.random(100) < 0.01
        s[hit] = (s[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
        reads.append((3 - s[::-1]) if r % 2 else s)
    return reads


def measure(ctx, k, contigs, reads, repeat):
    packed, start = readlib.pack_for_build(reads)
    rd = ctx.upload_reads(packed, start)
    g = api.Graph(ctx, ctx.build_sdbg(rd, k))
    seqs = [DNA[c].tobytes() for c in contigs]
    runs, scans = [], []
    for i in range(repeat + 1):                                               # (the first of each is the warm-up)
        st = g.pileup(rd, seqs)["stats"]
        sc = g.contig_sample_coverage(rd, [len(reads)], seqs)["stats"]
        if i:
            runs.append({n: v for n, v in st.items() if n.startswith("ms_")})
            scans.append(dict(ms_mark=sc["ms_mark"], ms_scan=sc["ms_scan"], ms_mass=sc["ms_mass"], ms_total=sc["ms_total"]))
    best = min(runs, key=lambda r: r["ms_total"])
    best_scan = min(scans, key=lambda r: r["ms_total"])
    placed = max(1, st["n_reads_placed"])
    line = dict(k=k, contigs=len(contigs), contig_letters=sum(c.size for c in contigs), reads=len(reads),
                stats={n: v for n, v in st.items() if not n.startswith("ms_")}, runs=runs, scans=scans, best=best, best_scan=best_scan,
                reads_per_s=len(reads) / (best["ms_total"] * 1e-3), scan_reads_per_s=len(reads) / (best_scan["ms_total"] * 1e-3),
                candidates_per_placed_read=st["n_candidates"] / placed, verified_per_placed_read=st["n_verified"] / placed,
                ratio_total=best["ms_total"] / best_scan["ms_total"], ratio_scan_phase=best["ms_scan"] / best_scan["ms_scan"] if best_scan["ms_scan"] > 0 else None)
    g.free()
    rd.free()
    return line


def main(argv):
    opt = {"--contigs": "20000", "--depth": "2", "--foreign": "0.2", "--k": "20", "--repeat": "3", "--out": ""}
    for a, v in zip(argv[0::2], argv[1::2]):
        if a not in opt:
            raise SystemExit(__doc__)
        opt[a] = v
    rng = np.random.default_rng(5)
    gene = rng.integers(0, 4, 900).astype(np.uint8)
    contigs = []
    for _ in range(int(opt["--contigs"])):
        s = variant(rng, gene)
        n = min(s.size, int(rng.integers(360, 541)))
        at = int(rng.integers(0, s.size - n + 1))
        contigs.append(s[at:at + n])
    ctx = api.Context(0)
    lines = []
    for what, only_foreign in (("reads drawn from the contigs", False), ("no read matches", True)):
        reads = make_reads(rng, contigs, float(opt["--depth"]), float(opt["--foreign"]), only_foreign)
        line = dict(input=what, depth=float(opt["--depth"]), foreign=1.0 if only_foreign else float(opt["--foreign"]),
                    **measure(ctx, int(opt["--k"]), contigs, reads, int(opt["--repeat"])))
        print(json.dumps(line), flush=True)
        lines.append(line)
    if opt["--out"]:
        with open(opt["--out"], "w") as fh:
            fh.write("".join(json.dumps(x) + "\n" for x in lines))
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1:])
