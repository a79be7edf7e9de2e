#!/usr/bin/env python3
"""The rate of mgta_seqs_nearest on a synthetic gene's worth of contigs and references.

python scripts/nearest_rate.py [--seqs 20000] [--refs 500] [--repeat 3] [--out profiles/nearest/run.json]

The references are `refs` variants of one random protein of 300 residues, 250 to 300 residues long; the contigs are pieces of
variants of the same protein, 120 to 180 residues long.  A variant has one residue in ten substituted and a few insertions and
deletions of 1 to 5 residues.  Scoring is 5 / -4, gap_open 10, gap_extend 1.  Printed per run: cell updates (L * R over all pairs) per
second of ms_score and cell updates (L * R over the traced pairs) per second of ms_trace (HIP events of the library), the peak device
memory of the call, what the runtime answered about residency (workgroups per CU, waves per workgroup, LDS bytes, segments) and the
number of trace batches.  The first call of a process pays the code object's load; the best of `repeat` calls is reported next to all
of them."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from megagta_amd import api, nearest  # noqa: E402

AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)


def variant(rng, protein: np.ndarray) -> np.ndarray:
    s = protein.copy()
    hit = rng.random(s.size) < 0.1
    s[hit] = AA[rng.integers(0, 20, int(hit.sum()))]
    for _ in range(int(rng.integers(0, 4))):
        at, k = int(rng.integers(5, s.size - 10)), int(rng.integers(1, 6))
        s = np.concatenate([s[:at], s[at + k:]]) if rng.random() < 0.5 else np.concatenate([s[:at], AA[rng.integers(0, 20, k)], s[at:]])
    return s


def piece(rng, s: np.ndarray, lo: int, hi: int) -> bytes:
    n = min(s.size, int(rng.integers(lo, hi + 1)))
    at = int(rng.integers(0, s.size - n + 1))
    return s[at:at + n].tobytes()


def main(argv):
    opt = {"--seqs": "20000", "--refs": "500", "--repeat": "3", "--out": ""}
    for a, v in zip(argv[0::2], argv[1::2]):
        if a not in opt:
            raise SystemExit(__doc__)
        opt[a] = v
    rng = np.random.default_rng(3)
    protein = AA[rng.integers(0, 20, 300)]
    refs = [piece(rng, variant(rng, protein), 250, 300) for _ in range(int(opt["--refs"]))]
    sub = nearest.match_mismatch(5, -4)
    ctx = api.Context(0)
    lines = []
    for n in [int(x) for x in opt["--seqs"].split(",")]:
        seqs = [piece(rng, variant(rng, protein), 120, 180) for _ in range(n)]
        runs = []
        for _ in range(int(opt["--repeat"])):
            t0 = time.time()
            res = ctx.nearest(seqs, refs, sub, 10, 1)
            st = res["stats"]
            runs.append(dict(ms_score=st["ms_score"], ms_trace=st["ms_trace"], wall_s=time.time() - t0))
        best, best_trace = min(r["ms_score"] for r in runs), min(r["ms_trace"] for r in runs)
        recs = res["recs"]
        ok = recs["status"] == 0
        cols = (recs["n_match"] + recs["n_insert"] + recs["n_delete"])[ok]
        line = dict(seqs=n, refs=len(refs), letters=sum(len(s) for s in seqs), ref_letters=sum(len(s) for s in refs),
                    stats={k: v for k, v in st.items() if not k.startswith("ms_")}, runs=runs, best_ms_score=best, best_ms_trace=best_trace,
                    score_cell_updates_per_s=st["n_cells"] / (best * 1e-3) if best > 0 else None,
                    trace_cell_updates_per_s=st["n_trace_cells"] / (best_trace * 1e-3) if best_trace > 0 else None,
                    peak_device_bytes=st["peak_bytes"], mean_identity=float(np.mean(recs["n_ident"][ok] / cols)) if ok.any() else None)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if opt["--out"]:
        with open(opt["--out"], "w") as fh:
            fh.write("".join(json.dumps(x) + "\n" for x in lines))
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1:])
