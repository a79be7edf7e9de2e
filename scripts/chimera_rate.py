#!/usr/bin/env python3
"""The rate of mgta_seqs_chimera next to mgta_seqs_nearest on the synthetic gene of scripts/nearest_rate.py.

python scripts/chimera_rate.py [--seqs 20000] [--refs 500] [--repeat 3] [--out profiles/chimera/run.json]

Contigs, references and scoring are those of scripts/nearest_rate.py (same seed, same construction: 120 to 180 residues against 250 to
300); min_seg 10, min_gain 15.  The yardstick is nearest's ms_score of the same process on the same input: the top-two pass computes
twice its cells (every pair in both directions), so the figure is ms_top / (2 * ms_score); 1.0 means a cell of the row-per-lane sweep
costs what a cell of the column-per-lane sweep costs.  Printed per run: that ratio from the best of `repeat` calls each, cell updates
per second of both passes, ms_parents, the peak device memory, what the runtime answered about residency and the counts per status."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from megagta_amd import api, nearest  # noqa: E402
from nearest_rate import AA, piece, variant  # noqa: E402


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
            near = ctx.nearest(seqs, refs, sub, 10, 1)
            t1 = time.time()
            res = ctx.chimera(seqs, refs, sub, 10, 1, 10, 15)
            st = res["stats"]
            runs.append(dict(ms_score=near["stats"]["ms_score"], ms_top=st["ms_top"], ms_parents=st["ms_parents"], nearest_wall_s=t1 - t0, chimera_wall_s=time.time() - t1))
        assert np.array_equal(res["recs"]["ref"], near["recs"]["ref"]) and np.array_equal(res["recs"]["score"], near["recs"]["score"])
        ms_score, ms_top, ms_par = (min(r[k] for r in runs) for k in ("ms_score", "ms_top", "ms_parents"))
        line = dict(seqs=n, refs=len(refs), letters=sum(len(s) for s in seqs), ref_letters=sum(len(s) for s in refs),
                    stats={k: v for k, v in st.items() if not k.startswith("ms_")}, runs=runs, best_ms_score=ms_score, best_ms_top=ms_top, best_ms_parents=ms_par,
                    top_over_twice_score=ms_top / (2 * ms_score) if ms_score > 0 else None,
                    nearest_cell_updates_per_s=near["stats"]["n_cells"] / (ms_score * 1e-3) if ms_score > 0 else None,
                    top_cell_updates_per_s=st["n_cells"] / (ms_top * 1e-3) if ms_top > 0 else None,
                    parents_cell_updates_per_s=st["n_parent_cells"] / (ms_par * 1e-3) if ms_par > 0 else None, peak_device_bytes=st["peak_bytes"])
        print(json.dumps(line), flush=True)
        lines.append(line)
    if opt["--out"]:
        with open(opt["--out"], "w") as fh:
            fh.write("".join(json.dumps(x) + "\n" for x in lines))
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1:])
