#!/usr/bin/env python3
"""The rate of mgta_seqs_frameshift beside mgta_seqs_nearest on the same contigs, in one process.

python scripts/frameshift_rate.py [--seqs 3000] [--refs 300] [--repeat 3] [--fasta nucl.fasta --ref ref.faa] [--out profiles/frameshift/run.json]

Synthetic input (the shape of scripts/nearest_rate.py, in nucleotides): the references are `refs` variants of one random protein of
300 residues, 250 to 300 residues long; the contigs are pieces of 300 residues of variants of the same protein, back-translated with
random synonymous codons: 900 nucleotides each, every third with one nucleotide deleted or inserted.  With --fasta and --ref the contigs
and references of those files are used instead.  Scoring is 5 / -4, gap_open 10, gap_extend 1, frameshift 10.  Printed: ms_score and
ms_trace of `frameshift` (HIP events of the library), ms_score of `nearest` on the frame-0 translations of the same contigs, their
ratio, cell updates per second of both, and what the runtime answered about residency.  The best of `repeat` calls is reported next
to all of them."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from megagta_amd import api, frameshift, nearest, synth  # noqa: E402
from nearest_rate import AA, piece, variant  # noqa: E402


def back_translate(rng, prot: bytes) -> str:
    out = []
    for a in prot.decode():
        c = int(rng.choice(synth.codons_for(a)))
        out.append("ACGT"[c >> 4] + "ACGT"[(c >> 2) & 3] + "ACGT"[c & 3])
    return "".join(out)


def main(argv):
    opt = {"--seqs": "3000", "--refs": "300", "--repeat": "3", "--out": "", "--fasta": "", "--ref": ""}
    for a, v in zip(argv[0::2], argv[1::2]):
        if a not in opt:
            raise SystemExit(__doc__)
        opt[a] = v
    rng = np.random.default_rng(3)
    if opt["--fasta"]:
        with open(opt["--fasta"], encoding="latin-1") as fh:
            nucl = [s for _, s in nearest.parse_fasta(fh.read())]
        refs = nearest.read_refs(opt["--ref"])[1]
    else:
        protein = AA[rng.integers(0, 20, 320)]
        refs = [piece(rng, variant(rng, protein), 250, 300).decode() for _ in range(int(opt["--refs"]))]
        nucl = []
        for k in range(int(opt["--seqs"])):
            x = back_translate(rng, piece(rng, variant(rng, protein), 300, 300))
            at = int(rng.integers(30, len(x) - 30))
            nucl.append(x if k % 3 else (x[:at] + x[at + 1:] if k % 2 else x[:at] + "ACGT"[int(rng.integers(4))] + x[at:]))
    prots = ["".join(frameshift.codon_residue(x[k:k + 3]) for k in range(0, len(x) - 2, 3)) for x in nucl]
    sub = nearest.match_mismatch(5, -4)
    ctx = api.Context(0)
    runs = []
    for _ in range(int(opt["--repeat"])):
        fs = ctx.frameshift(nucl, refs, sub, 10, 1, 10)
        nr = ctx.nearest(prots, refs, sub, 10, 1)
        runs.append(dict(ms_score=fs["stats"]["ms_score"], ms_trace=fs["stats"]["ms_trace"], nearest_ms_score=nr["stats"]["ms_score"],
                         nearest_ms_trace=nr["stats"]["ms_trace"]))
    best = {k: min(r[k] for r in runs) for k in runs[0]}
    st, nst = fs["stats"], nr["stats"]
    line = dict(seqs=len(nucl), refs=len(refs), nucleotides=sum(map(len, nucl)), ref_letters=sum(map(len, refs)),
                stats={k: v for k, v in st.items() if not k.startswith("ms_")}, nearest_cells=nst["n_cells"], runs=runs, best=best,
                score_ratio_to_nearest=best["ms_score"] / best["nearest_ms_score"] if best["nearest_ms_score"] > 0 else None,
                score_cell_updates_per_s=st["n_cells"] / (best["ms_score"] * 1e-3) if best["ms_score"] > 0 else None,
                nearest_cell_updates_per_s=nst["n_cells"] / (best["nearest_ms_score"] * 1e-3) if best["nearest_ms_score"] > 0 else None)
    print(json.dumps(line), flush=True)
    if opt["--out"]:
        with open(opt["--out"], "w") as fh:
            fh.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1:])
