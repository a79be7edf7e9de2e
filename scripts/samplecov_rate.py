#!/usr/bin/env python3
"""The read scan of mgta_contig_sample_coverage beside the read walk of mgta_reads_match_contigs, on one input and in one process.

python scripts/samplecov_rate.py [--reads 2000000] [--k 44] [--libs 4] [--out profiles/samplecov/run.json]

The bench's synthetic reads (synth.make_metagenome_device, 150 bp, one gene) are drawn on the device, their `-m 1` graph is built and
loaded where it lies, and the contigs are the gene's copies in the sample's genomes, as in scripts/matchreads_rate.py.  The reads are
cut into `libs` libraries of equal size.  Printed and written: the walk of match_reads(counts=True) and the scan of
contig_sample_coverage (both walk every window of every read), the mark and mass times, read windows per second and the ratio of
the two scans, all from the library's HIP events."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before the first call into the library: one HIP runtime serves both)

from megagta_amd import api, synth  # noqa: E402

DNA = "ACGT"


def main(argv):
    n_reads, k, n_libs, out_path = 2_000_000, 44, 4, None
    it = iter(argv)
    for a in it:
        if a == "--reads":
            n_reads = int(next(it))
        elif a == "--k":
            k = int(next(it))
        elif a == "--libs":
            n_libs = int(next(it))
        elif a == "--out":
            out_path = next(it)
        else:
            print(__doc__)
            return 2
    ctx = api.Context(0)
    mg = synth.make_metagenome_device(n_reads, 150, (("rplB", 277),), seed=1000 + n_reads % 997, host_sample=0)
    rd = ctx.adopt_reads(mg.packed.data_ptr(), mg.n_words, mg.start.data_ptr(), mg.n_reads, keepalive=(mg.packed, mg.start))
    build = ctx.build_sdbg(rd, k, collect=False).stats
    g = api.Graph(ctx, None)
    contigs = ["".join(DNA[c] for c in v) for v in mg.genes[0].variants]
    lib_end = [n_reads * (s + 1) // n_libs for s in range(n_libs)]
    warm = [min(n_reads, 100000)]
    g.match_reads(rd, contigs, n_short_reads=warm[0], counts=True)         # warm: the marks, the code objects
    g.contig_sample_coverage(rd, warm, contigs)
    res = dict(reads=n_reads, k=k, edges=g.size, contigs=len(contigs), libs=n_libs, lib_end=lib_end, build_passes=build["n_passes"], runs=[])
    for _ in range(3):
        m = g.match_reads(rd, contigs, counts=True)
        s = g.contig_sample_coverage(rd, lib_end, contigs)
        ms, ss = m["stats"], s["stats"]
        assert int(m["hit_windows"].astype("uint64").sum()) == ss["n_hit_windows"] == int(s["lib_hit_windows"].sum())   # the two scans saw the same hits
        res["runs"].append(dict(match=ms, sample=ss, scan_over_walk=ss["ms_scan"] / ms["ms_walk"],
                                match_read_windows_per_s=ms["n_read_windows"] / (ms["ms_walk"] * 1e-3),
                                sample_read_windows_per_s=ss["n_read_windows"] / (ss["ms_scan"] * 1e-3),
                                hit_share=ss["n_hit_windows"] / max(1, ss["n_read_windows"])))
    text = json.dumps(res, indent=1)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
