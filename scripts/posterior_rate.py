#!/usr/bin/env python3
"""The rate of mgta_seqs_posterior on a synthetic gene's worth of contigs, next to mgta_seqs_align's fill on the same input.

python scripts/posterior_rate.py [--seqs 100000] [--model-len 277] [--contig-len 150] [--repeat 3] [--out profiles/posterior/run.json]

The model and the contigs are those of scripts/align_rate.py (same generator, same seeds).  Per run, in one session: the Viterbi
placement (its ms_fill), then the posteriors of the labels its paths give.  Printed: ms_forward and ms_backward (HIP events of the
library), cell updates (L * M) per second of each and of both, the same for align_fill_kernel and the ratio of the two, what the runtime
answered about residency and the peak device memory of the call.  The first call of a process pays the code object's load; the best of
`repeat` calls is reported next to all of them."""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from megagta_amd import api, hmm, posterior, synth  # noqa: E402
from align_rate import AA, make_contigs  # noqa: E402


def main(argv):
    opt = {"--seqs": "100000", "--model-len": "277", "--contig-len": "150", "--repeat": "3", "--out": ""}
    for a, v in zip(argv[0::2], argv[1::2]):
        if a not in opt:
            raise SystemExit(__doc__)
        opt[a] = v
    rng = np.random.default_rng(3)
    protein = AA[rng.integers(0, 20, int(opt["--model-len"]))]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "model.hmm")
        with open(path, "w") as fh:
            fh.write(synth.hmm_text("rate", protein.tobytes().decode().upper()))
        model = hmm.parse_hmm(path)
    ctx = api.Context(0)
    dev = api.DeviceHmm(ctx, model)
    lines = []
    for n in [int(x) for x in opt["--seqs"].split(",")]:
        seqs = make_contigs(n, protein, int(opt["--contig-len"]))
        runs = []
        for _ in range(int(opt["--repeat"])):
            t0 = time.time()
            ares = ctx.align(dev, seqs, cols=True, paths=True)
            t1 = time.time()
            labels = posterior.labels_of(ares, seqs)
            t2 = time.time()
            res = ctx.posterior(dev, seqs, labels=labels, cols=True)
            st = res["stats"]
            runs.append(dict(ms_forward=st["ms_forward"], ms_backward=st["ms_backward"], ms_fill=ares["stats"]["ms_fill"], align_wall_s=t1 - t0,
                             posterior_wall_s=time.time() - t2))
        best = min(runs, key=lambda r: r["ms_forward"] + r["ms_backward"])
        fill = min(r["ms_fill"] for r in runs)
        cells = st["n_cells"]
        pps = np.concatenate(res["pp"]) if n else np.zeros(0)
        line = dict(seqs=n, model_len=model.M, letters=sum(len(s) for s in seqs), stats={k: v for k, v in st.items() if not k.startswith("ms_")}, runs=runs,
                    best_ms_forward=best["ms_forward"], best_ms_backward=best["ms_backward"], best_ms_fill=fill,
                    forward_cells_per_s=cells / (best["ms_forward"] * 1e-3), backward_cells_per_s=cells / (best["ms_backward"] * 1e-3),
                    posterior_cells_per_s=cells / ((best["ms_forward"] + best["ms_backward"]) * 1e-3), align_fill_cells_per_s=cells / (fill * 1e-3),
                    ms_posterior_over_ms_fill=(best["ms_forward"] + best["ms_backward"]) / fill,
                    mean_pp=float(pps.mean()) if pps.size else None, share_below_half=float((pps < 0.5).mean()) if pps.size else None,
                    mean_fwd_minus_viterbi=float(np.mean((res["recs"]["fwd"] - ares["recs"]["score"])[res["recs"]["status"] == 0])) if st["n_scored"] else None)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if opt["--out"]:
        with open(opt["--out"], "w") as fh:
            fh.write("".join(json.dumps(x) + "\n" for x in lines))
    dev.free()
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1:])
