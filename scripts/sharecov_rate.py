#!/usr/bin/env python3
"""What mgta_contig_share_coverage costs beside mgta_contig_coverage, and how its count phase takes redundant contigs.

python scripts/sharecov_rate.py <sdbg_prefix> <contigs.fasta> [more.fasta ...] [--out profiles/taxonabund/run.json]
python scripts/sharecov_rate.py --synthetic N_READS [--out ...]

<sdbg_prefix>: the graph files of a finished run's last k (out/k44/44); the FASTA files: contigs/<gene>/nucl_merged.fasta of its genes
(the input of scripts/coverage_rate.py).  --synthetic builds its own input in the process instead: N_READS reads of 150 bp from a random
genome of N_READS * 5 bp (coverage 30), a graph of k = 44 from them, and the distinct reads as the contigs.

Every contig is put into the call 1x, 10x and 100x (100x only while the call stays under 2^32 windows), once with the copies of a
contig side by side ("blocked") and once as whole sets one after the other ("interleaved").  Both calls run in this one process on
the same contigs; the numbers are the library's HIP events: ms_walk of both, the count phase and the share phase, the ratio
ms_total(share) / ms_kernel(coverage), and the bytes the share call keeps per window (table + slot numbers; 8 more per window of a
batch for the edge ids).  Equal ids are added up inside a wave before the atomic when they meet in one: blocked copies do, interleaved
ones do not -- the difference between the two rows is what that aggregation is worth, and the growth of ms_count per window from 1x to
100x in the interleaved rows is what contention on one address costs without it."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from megagta_amd import api, coverage as cv, synth  # noqa: E402


def synthetic(ctx, n_reads):
    rng = np.random.default_rng(7)
    genome = rng.integers(0, 4, n_reads * 5, dtype=np.uint8)
    pos = rng.integers(0, genome.size - 150 + 1, n_reads)
    reads = np.stack([genome[p:p + 150] for p in pos])
    packed, start = synth.pack_reads_for_build(reads)
    ctx.build_sdbg(ctx.upload_reads(packed, start), 44, collect=False)
    g = api.Graph(ctx, None, keep_multiplicity=True)
    seqs = list(dict.fromkeys("".join("ACGT"[c] for c in r) for r in reads))
    return g, seqs


def measure(g, seqs):
    g.contig_coverage(seqs[:1000], abundance=False)
    g.contig_share_coverage(seqs[:1000])                                  # warm: scratch, code objects
    t = time.time()
    cov = g.contig_coverage(seqs, abundance=False)["stats"]
    t_cov = time.time() - t
    t = time.time()
    sh = g.contig_share_coverage(seqs)["stats"]
    t_sh = time.time() - t
    w = max(1, sh["n_windows"])
    return dict(contigs=len(seqs), windows=sh["n_windows"], distinct_edges=sh["n_distinct_edges"], windows_per_edge=sh["n_covered"] / max(1, sh["n_distinct_edges"]),
                cov_ms_walk=cov["ms_walk"], cov_ms_kernel=cov["ms_kernel"], share_ms_walk=sh["ms_walk"], share_ms_count=sh["ms_count"], share_ms_share=sh["ms_share"],
                share_ms_total=sh["ms_total"], ratio_total_to_cov_kernel=sh["ms_total"] / max(1e-9, cov["ms_kernel"]), walk_ratio=sh["ms_walk"] / max(1e-9, cov["ms_walk"]),
                ns_count_per_window=sh["ms_count"] * 1e6 / w, ns_share_per_window=sh["ms_share"] * 1e6 / w, table_bytes=sh["table_bytes"],
                kept_bytes_per_window=(sh["table_bytes"] + sh["window_bytes"]) / w, batches=sh["n_batches"], cov_wall_s=t_cov, share_wall_s=t_sh)


def main(argv):
    out_path = None
    if "--out" in argv:
        i = argv.index("--out")
        out_path = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    ctx = api.Context(0)
    if len(argv) == 2 and argv[0] == "--synthetic":
        g, seqs = synthetic(ctx, int(argv[1]))
        res = {"synthetic_reads": int(argv[1])}
    elif len(argv) >= 2:
        g = api.Graph.from_files(ctx, argv[0], keep_multiplicity=True)
        seqs = [s for fa in argv[1:] for s in cv.read_fasta(fa)[1]]
        res = {"sdbg_prefix": argv[0], "fastas": argv[1:]}
    else:
        print(__doc__)
        return 2
    res.update(edges=g.size, k=g.k)
    windows = sum(max(0, len(s) - g.k) for s in seqs)
    runs = []
    for copies in (1, 10, 100):
        if windows * copies >= 1 << 32:
            break
        for layout in ("blocked", "interleaved") if copies > 1 else ("once",):
            call = [s for s in seqs for _ in range(copies)] if layout == "blocked" else seqs * copies
            runs.append(dict(copies=copies, layout=layout, **measure(g, call)))
            print(json.dumps(runs[-1]), flush=True)
    res["runs"] = runs
    text = json.dumps(res, indent=1)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
