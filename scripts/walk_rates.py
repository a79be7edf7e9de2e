#!/usr/bin/env python3
"""Repeated calls of the stages whose rate scripts measure one call only, for a comparison of two builds of the library.

MEGAGTA_HIP_LIB=<path of a libmegagta_hip.so> python scripts/walk_rates.py OUT.json

contig_coverage (with and without abundance) and contig_share_coverage on the synthetic input of scripts/sharecov_rate.py
(--synthetic 200000), match_reads (bits only and with counts) on the inputs of scripts/matchreads_rate.py (1 M and 10 M reads,
k = 44): one warm-up, then REPEAT measured calls each, the library's own HIP-event times of every call.  Run it once per build in
one session; scripts/pileup_rate.py, samplecov_rate.py and phase_rate.py list their measured calls themselves.
profiles/walk/README.md records such a comparison."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch  # noqa: E402,F401

from megagta_amd import api, synth  # noqa: E402
import sharecov_rate  # noqa: E402

REPEAT = 5
DNA = "ACGT"


def ms(st):
    return {n: v for n, v in st.items() if n.startswith("ms_")}


def main(out):
    res = {"lib": os.environ.get("MEGAGTA_HIP_LIB", "default")}
    ctx = api.Context(0)
    g, seqs = sharecov_rate.synthetic(ctx, 200000)
    res["coverage_input"] = dict(contigs=len(seqs), edges=g.size, k=g.k)
    for name, call in (("coverage_abundance", lambda: g.contig_coverage(seqs)), ("coverage", lambda: g.contig_coverage(seqs, abundance=False)),
                       ("share", lambda: g.contig_share_coverage(seqs))):
        call()
        res[name] = [ms(call()["stats"]) for _ in range(REPEAT)]
        print(name, json.dumps(res[name]), flush=True)
    g.free()
    ctx.release_scratch()
    for n_reads in (1_000_000, 10_000_000):
        mg = synth.make_metagenome_device(n_reads, 150, (("rplB", 277),), seed=1000 + n_reads % 997, host_sample=0)
        rd = ctx.adopt_reads(mg.packed.data_ptr(), mg.n_words, mg.start.data_ptr(), mg.n_reads, keepalive=(mg.packed, mg.start))
        ctx.build_sdbg(rd, 44, collect=False)
        g = api.Graph(ctx, None)
        contigs = ["".join(DNA[c] for c in v) for v in mg.genes[0].variants]
        g.match_reads(rd, contigs, n_short_reads=min(n_reads, 100000))
        for name, counts in (("bits_only", False), ("counts", True)):
            g.match_reads(rd, contigs, counts=counts)
            key = f"match_{n_reads}_{name}"
            res[key] = [ms(g.match_reads(rd, contigs, counts=counts)["stats"]) for _ in range(REPEAT)]
            print(key, json.dumps(res[key]), flush=True)
        g.free()
        rd.free()
        ctx.release_scratch()
        del mg
        torch.cuda.empty_cache()
    with open(out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1])
