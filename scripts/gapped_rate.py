#!/usr/bin/env python3
"""ms_scan of mgta_reads_pileup_gapped beside ms_scan of mgta_reads_pileup: the same graph, reads and contigs, one process.

python scripts/gapped_rate.py [--contigs 2000] [--depth 2] [--foreign 0.2] [--k 20] [--repeat 3] [--entry both|pileup] [--out profiles/gapped/run.json]

The contigs and the reads are those of scripts/pileup_rate.py (variants of one random gene, reads of 100 letters with 1 % substitutions).
Two inputs: the reads as they are (none was made with an insertion or deletion), and the same reads with one in a hundred of those
drawn from a contig carrying one insertion or deletion of 1 to 5 letters between its letters 30 and 70.  Per input one JSON line: all
ms_scan of `repeat` calls of either entry after a warm-up, the best of each, their ratio and the gapped counters.  `--entry pileup`
times mgta_reads_pileup alone; with MEGAGTA_HIP_LIB naming a library built from another commit it gives that commit's figure."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from megagta_amd import _lib  # noqa: E402
from pileup_rate import DNA, make_reads, variant  # noqa: E402


def with_indels(rng, reads, share):
    out, n = [], 0
    for r in reads:
        if rng.random() < share:
            at, m = int(rng.integers(30, 71)), int(rng.integers(1, 6))
            r = np.concatenate([r[:at], r[at + m:]]) if rng.random() < 0.5 else np.concatenate([r[:at], rng.integers(0, 4, m).astype(np.uint8), r[at:]])
            n += 1
        out.append(r)
    return out, n


def measure(ctx, api, readlib, k, contigs, reads, repeat, both):
    rd = ctx.upload_reads(*readlib.pack_for_build(reads))
    g = api.Graph(ctx, ctx.build_sdbg(rd, k))
    seqs = [DNA[c].tobytes() for c in contigs]
    plain, gapped, gst = [], [], {}
    for i in range(repeat + 1):                                               # (the first of each is the warm-up)
        st = g.pileup(rd, seqs)["stats"]
        if i:
            plain.append(st["ms_scan"])
        if both:
            gst = g.pileup_gapped(rd, seqs)["stats"]
            if i:
                gapped.append(gst["ms_scan"])
    g.free()
    rd.free()
    line = dict(k=k, contigs=len(contigs), reads=len(reads), pileup_ms_scan=plain, pileup_best=min(plain), n_candidates=st["n_candidates"],
                n_verified=st["n_verified"], n_reads_placed=st["n_reads_placed"])
    if both:
        line.update(gapped_ms_scan=gapped, gapped_best=min(gapped), ratio=min(gapped) / min(plain),
                    gapped_stats={n: v for n, v in gst.items() if n.startswith("n_gap") or n in ("n_reads_gapped", "n_inserted", "n_deleted", "diag_list_entries",
                                                                                                "n_reads_placed", "groups_per_cu", "peak_bytes")})
    return line


def main(argv):
    opt = {"--contigs": "2000", "--depth": "2", "--foreign": "0.2", "--k": "20", "--repeat": "3", "--entry": "both", "--out": ""}
    for a, v in zip(argv[0::2], argv[1::2]):
        if a not in opt:
            raise SystemExit(__doc__)
        opt[a] = v
    both = opt["--entry"] == "both"
    if not both:
        _lib.SYMBOLS.pop("mgta_reads_pileup_gapped", None)                    # (a library of a commit before the entry)
    from megagta_amd import api, readlib
    rng = np.random.default_rng(5)
    gene = rng.integers(0, 4, 900).astype(np.uint8)
    contigs = []
    for _ in range(int(opt["--contigs"])):
        s = variant(rng, gene)
        n = min(s.size, int(rng.integers(360, 541)))
        at = int(rng.integers(0, s.size - n + 1))
        contigs.append(s[at:at + n])
    reads = make_reads(rng, contigs, float(opt["--depth"]), float(opt["--foreign"]), False)
    ctx = api.Context(0)
    lines = []
    for what, share in (("no read with an insertion or deletion", 0.0), ("1 % of the reads with one", 0.01)):
        rs, n = with_indels(np.random.default_rng(7), reads, share)
        line = dict(input=what, reads_changed=n, library=os.environ.get("MEGAGTA_HIP_LIB", ""), **measure(ctx, api, readlib, int(opt["--k"]), contigs, rs, int(opt["--repeat"]), both))
        print(json.dumps(line), flush=True)
        lines.append(line)
    if opt["--out"]:
        with open(opt["--out"], "w") as fh:
            fh.write("".join(json.dumps(x) + "\n" for x in lines))
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1:])
