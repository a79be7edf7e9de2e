#!/usr/bin/env python3
"""The rate of mgta_reads_phase next to the read scan of mgta_reads_pileup: the same reads and contigs, one process.

python scripts/phase_rate.py [--contigs 20000] [--depth 2] [--foreign 0.2] [--k 20] [--repeat 3] [--min-depth 4] [--out profiles/phase/run.json]

The input is that of scripts/pileup_rate.py (its first one: reads drawn from the contigs) with a fifth of the reads as mates: library 0
is paired and holds a fifth of the reads, each pair two reads of 100 letters from one contig in opposite orientations; library 1 holds
the rest, single-end.  Graph.pileup(per_read=True) runs once after a warm-up and gives the placements; the sites are the positions its
counts list as variants at --min-depth (pileup.variant_mask).  Context.phase then runs `repeat` times after a warm-up.  One JSON line:
the stats of both, ms_upload and ms_scan of the best phase call, ms_scan of the pileup call, the ratio of the two scans and fragment
slots per second of the phase scan."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from megagta_amd import api, phase, readlib  # noqa: E402
from pileup_rate import DNA, make_reads, variant  # noqa: E402


def make_mates(rng, contigs, n_pairs: int):
    reads = []
    for _ in range(n_pairs):
        c = contigs[int(rng.integers(0, len(contigs)))]
        flip = rng.random() < 0.5
        for mate in (0, 1):
            at = int(rng.integers(0, c.size - 100 + 1))
            s = c[at:at + 100].copy()
            hit = rng.random(100) < 0.01
            s[hit] = (s[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
            reads.append((3 - s[::-1]) if (mate == 1) != flip else s)
    return reads


def main(argv):
    opt = {"--contigs": "20000", "--depth": "2", "--foreign": "0.2", "--k": "20", "--repeat": "3", "--min-depth": "4", "--out": ""}
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
    single = make_reads(rng, contigs, float(opt["--depth"]), float(opt["--foreign"]), False)
    n_pairs = len(single) // 10
    reads = make_mates(rng, contigs, n_pairs) + single[:len(single) - 2 * n_pairs]
    libs = [(2 * n_pairs, True), (len(reads), False)]
    ctx = api.Context(0)
    rd = ctx.upload_reads(*readlib.pack_for_build(reads))
    g = api.Graph(ctx, ctx.build_sdbg(rd, int(opt["--k"])))
    seqs = [DNA[c].tobytes() for c in contigs]
    g.pileup(rd, seqs)                                                        # (the warm-up)
    pile = g.pileup(rd, seqs, per_read=True)
    sites = phase.sites_from_pileup([s.decode() for s in seqs], pile, min_depth=int(opt["--min-depth"]))
    runs = []
    for i in range(int(opt["--repeat"]) + 1):
        res = ctx.phase(rd, pile["reads"], libs, seqs, sites)
        if i:
            runs.append({n: v for n, v in res["stats"].items() if n.startswith("ms_")})
    best = min(runs, key=lambda r: r["ms_scan"])
    st = res["stats"]
    slots = n_pairs + len(reads) - 2 * n_pairs
    line = dict(k=int(opt["--k"]), contigs=len(contigs), contig_letters=sum(c.size for c in contigs), reads=len(reads), pairs_of_mates=n_pairs,
                min_depth=int(opt["--min-depth"]), stats={n: v for n, v in st.items() if not n.startswith("ms_")}, runs=runs, best=best,
                pileup_stats={n: v for n, v in pile["stats"].items() if not n.startswith("ms_")}, pileup_ms_scan=pile["stats"]["ms_scan"],
                pileup_ms_total=pile["stats"]["ms_total"], ratio_scan=best["ms_scan"] / pile["stats"]["ms_scan"],
                slots_per_s=slots / (best["ms_scan"] * 1e-3), place_bytes=24 * len(reads))
    print(json.dumps(line), flush=True)
    if opt["--out"]:
        with open(opt["--out"], "w") as fh:
            fh.write(json.dumps(line) + "\n")
    g.free()
    rd.free()
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1:])
