#!/usr/bin/env python3
"""The rate of mgta_seqs_align on a synthetic gene's worth of contigs.

python scripts/align_rate.py [--seqs 100000] [--model-len 277] [--contig-len 150] [--repeat 3] [--out profiles/align/run.json]

The model is synth.hmm_text over a random protein of `model-len` residues; the contigs are pieces of that protein of `contig-len`
residues give or take a fifth, one residue in twenty substituted, one contig in ten with a deletion and one in ten with an insertion
of 1 to 5 residues.  Printed per run: cell updates (L * M) per second of ms_fill, ms_fill and ms_trace (HIP events of the library),
what the runtime answered about residency (workgroups per CU, waves per workgroup, LDS bytes, whether the match scores sat in LDS)
and the number of batches.  The first call of a process pays the code object's load; the best of `repeat` calls is reported next to
all of them."""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from megagta_amd import api, hmm, synth  # noqa: E402

AA = np.frombuffer(b"acdefghiklmnpqrstvwy", dtype=np.uint8)


def make_contigs(n: int, protein: np.ndarray, contig_len: int, seed: int = 7) -> list[bytes]:
    rng = np.random.default_rng(seed)
    M = protein.size
    lens = np.minimum(M, rng.integers(max(1, contig_len - contig_len // 5), contig_len + contig_len // 5 + 1, n))
    starts = (rng.random(n) * (M - lens + 1)).astype(np.int64)
    kind = rng.integers(0, 10, n)                                        # 0: a deletion, 1: an insertion
    out = []
    for i in range(n):
        s = protein[starts[i]:starts[i] + lens[i]].copy()
        hit = rng.random(s.size) < 0.05
        s[hit] = AA[rng.integers(0, 20, int(hit.sum()))]
        if kind[i] < 2 and s.size > 20:
            at, k = int(rng.integers(5, s.size - 10)), int(rng.integers(1, 6))
            s = np.concatenate([s[:at], s[at + k:]]) if kind[i] == 0 else np.concatenate([s[:at], AA[rng.integers(0, 20, k)], s[at:]])
        out.append(s.tobytes())
    return out


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
            res = ctx.align(dev, seqs, cols=True, paths=False)
            st = res["stats"]
            runs.append(dict(ms_fill=st["ms_fill"], ms_trace=st["ms_trace"], wall_s=time.time() - t0))
        best = min(r["ms_fill"] for r in runs)
        line = dict(seqs=n, model_len=model.M, letters=sum(len(s) for s in seqs), stats={k: v for k, v in st.items() if not k.startswith("ms_")}, runs=runs,
                    best_ms_fill=best, cell_updates_per_s=st["n_cells"] / (best * 1e-3) if best > 0 else None,
                    mean_score=float(np.mean(res["recs"]["score"][res["recs"]["status"] == 0])) if st["n_aligned"] else None)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if opt["--out"]:
        with open(opt["--out"], "w") as fh:
            fh.write("".join(json.dumps(x) + "\n" for x in lines))
    dev.free()
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1:])
