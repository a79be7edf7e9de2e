#!/usr/bin/env python3
"""The rate of mgta_reads_recruit on a synthetic metagenome.

python scripts/recruit_rate.py [--reads 400000] [--model-len 300] [--read-len 150] [--min-aa 20] [--repeat 6] [--chunk 0] [--out profiles/recruit/run.json] [--local]

The reads are synth.make_metagenome's (random genomes of 20 kb, one diverged copy of the gene in each, both strands, substitution
errors), the model synth.hmm_text over the gene's consensus.  Printed per run: cell updates (aa_len * M over the scored frames) per
second of ms_fill, which holds translation, fill and records; ms_scan; the mean length of a scored stretch and the scored frames per
read (what `align_rate.py --contig-len` has to be given for sequences of the same lengths); what the runtime answered about residency;
the recruited share.  --local measures local mode (every stop-free stretch, the best placement of any substring); its line carries
"mode": "local".  The first call of a process pays the code object's load: it is listed with the others and left out of `best` and
`spread`, which are over the calls behind it."""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from megagta_amd import api, hmm, synth  # noqa: E402


def main(argv):
    opt = {"--reads": "400000", "--model-len": "300", "--read-len": "150", "--min-aa": "20", "--repeat": "6", "--chunk": "0", "--out": ""}
    local = "--local" in argv
    argv = [a for a in argv if a != "--local"]
    if len(argv) % 2:
        raise SystemExit(__doc__)
    for a, v in zip(argv[0::2], argv[1::2]):
        if a not in opt:
            raise SystemExit(__doc__)
        opt[a] = v
    lines = []
    ctx = api.Context(0)
    ctx.set_recruit_chunk(int(opt["--chunk"]))
    for n in [int(x) for x in opt["--reads"].split(",")]:
        mg = synth.make_metagenome(n, int(opt["--read-len"]), (("g", int(opt["--model-len"])),), seed=3)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "model.hmm")
            with open(path, "w") as fh:
                fh.write(synth.hmm_text("rate", mg.genes[0].consensus))
            model = hmm.parse_hmm(path)
        dev = api.DeviceHmm(ctx, model)
        rd = ctx.upload_reads(*synth.pack_reads_for_build(mg.reads))
        runs = []
        for _ in range(int(opt["--repeat"])):
            t0 = time.time()
            res = ctx.recruit(dev, rd, params=dict(min_aa=int(opt["--min-aa"]), local=local))
            st = res["stats"]
            runs.append(dict(ms_fill=st["ms_fill"], ms_scan=st["ms_scan"], wall_s=time.time() - t0))
        measured = [r["ms_fill"] for r in runs[1:]] or [runs[0]["ms_fill"]]
        best = min(measured)
        line = dict(mode="local" if local else "global", reads=n, model_len=model.M, read_len=int(opt["--read-len"]), stats={k: v for k, v in st.items() if not k.startswith("ms_")}, runs=runs,
                    best_ms_fill=best, spread_ms_fill=max(measured) - best, cell_updates_per_s=st["n_cells"] / (best * 1e-3) if best > 0 else None,
                    reads_per_s=n / (best * 1e-3) if best > 0 else None, mean_stretch=st["n_cells"] / model.M / max(1, st["n_frames_scored"]),
                    frames_per_read=st["n_frames_scored"] / n, recruited_share=st["n_recruited"] / n)
        print(json.dumps(line), flush=True)
        lines.append(line)
        rd.free()
        dev.free()
    if opt["--out"]:
        with open(opt["--out"], "w") as fh:
            fh.write("".join(json.dumps(x) + "\n" for x in lines))
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1:])
