#!/usr/bin/env python3
"""The rate of mgta_rows_pairs / mgta_rows_cluster on a synthetic gene's worth of aligned rows, next to the same pair counts in numpy.

python scripts/cluster_rate.py [--rows 20000] [--cols 300] [--span 150] [--cutoff 0.01] [--min-overlap 25] [--host-rows 2000]
                               [--repeat 3] [--out profiles/cluster/run.json]

The rows are fragments of `--span` columns, give or take a fifth, of 50 variants of one random protein of `--cols` residues (a variant
differs from it in 3 % of the columns), each fragment with one residue in 200 substituted; everything outside the fragment is `-`.
Printed: row pairs per second of ms_pairs (HIP events of the library: layout, pairs, count, scan, write over all tiles), ms_pairs and
ms_link, the peak device memory of the call, what the runtime answered about residency, and the numpy rate on the first `--host-rows`
rows (one row against all later ones per step: overlap and difference counts of the contract, vectorised).  The first call of a
process pays the code object's load; the best of `repeat` calls is reported next to all of them."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from megagta_amd import api  # noqa: E402

AA = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
GAP = 45


def make_rows(n: int, M: int, span: int, seed: int = 7) -> np.ndarray:
    rng = np.random.default_rng(seed)
    protein = AA[rng.integers(0, 20, M)]
    variants = np.repeat(protein[None, :], 50, axis=0)
    hit = rng.random(variants.shape) < 0.03
    variants[hit] = AA[rng.integers(0, 20, int(hit.sum()))]
    rows = variants[rng.integers(0, 50, n)].copy()
    hit = rng.random(rows.shape) < 0.005
    rows[hit] = AA[rng.integers(0, 20, int(hit.sum()))]
    lens = np.minimum(M, rng.integers(max(1, span - span // 5), span + span // 5 + 1, n))
    starts = (rng.random(n) * (M - lens + 1)).astype(np.int64)
    col = np.arange(M)[None, :]
    rows[(col < starts[:, None]) | (col >= (starts + lens)[:, None])] = GAP
    return rows


def host_pairs(rows: np.ndarray, min_overlap: int, cutoff: float):
    """the contract's pair counts, one row against all later ones per step -> (kept pairs, seconds)"""
    res = rows != GAP
    kept = 0
    t0 = time.time()
    for i in range(rows.shape[0] - 1):
        both = res[i + 1:] & res[i]
        n_overlap = both.sum(axis=1)
        n_diff = (both & (rows[i + 1:] != rows[i])).sum(axis=1)
        kept += int(((n_overlap >= min_overlap) & (n_diff.astype(np.float64) <= cutoff * n_overlap.astype(np.float64))).sum())
    return kept, time.time() - t0


def main(argv):
    opt = {"--rows": "20000", "--cols": "300", "--span": "150", "--cutoff": "0.01", "--min-overlap": "25", "--host-rows": "2000", "--repeat": "3", "--out": ""}
    for a, v in zip(argv[0::2], argv[1::2]):
        if a not in opt:
            raise SystemExit(__doc__)
        opt[a] = v
    n, M, cutoff, min_overlap = int(opt["--rows"]), int(opt["--cols"]), float(opt["--cutoff"]), int(opt["--min-overlap"])
    rows = make_rows(n, M, int(opt["--span"]))
    lens = (rows != GAP).sum(axis=1)
    ctx = api.Context(0)
    runs = []
    for _ in range(int(opt["--repeat"])):
        t0 = time.time()
        res = ctx.cluster(rows, lens, min_overlap, cutoff)
        st = res["stats"]
        runs.append(dict(ms_pairs=st["ms_pairs"], ms_link=st["ms_link"], wall_s=time.time() - t0))
    best = min(r["ms_pairs"] for r in runs)
    n_pairs = n * (n - 1) // 2
    h = min(n, int(opt["--host-rows"]))
    host_kept, host_s = host_pairs(rows[:h], min_overlap, cutoff)
    dev_kept_h = len(ctx.row_pairs(rows[:h], min_overlap, cutoff)["pairs"])
    line = dict(rows=n, cols=M, span=int(opt["--span"]), cutoff=cutoff, min_overlap=min_overlap, row_pairs=n_pairs,
                stats={k: v for k, v in st.items() if not k.startswith("ms_")}, runs=runs, best_ms_pairs=best,
                device_row_pairs_per_s=n_pairs / (best * 1e-3) if best > 0 else None, ms_link=min(r["ms_link"] for r in runs),
                peak_device_bytes=st["peak_bytes"], host_rows=h, host_seconds=host_s, host_row_pairs_per_s=h * (h - 1) // 2 / host_s if host_s > 0 else None,
                host_kept=host_kept, device_kept_on_host_rows=dev_kept_h)
    print(json.dumps(line), flush=True)
    assert host_kept == dev_kept_h, "numpy and the device disagree on the sample"
    if opt["--out"]:
        with open(opt["--out"], "w") as fh:
            fh.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1:])
