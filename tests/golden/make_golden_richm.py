#!/usr/bin/env python3
"""Goldens for POSITION-SPECIFIC profile HMMs (tests/rich_models.py): every other golden model has one transition row for all its
nodes and two-valued match columns, so a table read one node off is invisible in it.  Everything comes from the COMPILED REFERENCE
(oracle/_ref/megagta + probe), as in make_golden_bigm.py:

    python tests/golden/make_golden_richm.py

Reads and models are regenerated from their seeds by the tests (an md5 of every input is stored and checked); the model texts of r75
and r130 are our own generator's output and are committed beside the reference's parsed tables of them.  Per case: seeds from the
reference's `findstart`, per-seed cold (r75: and sequential warm) A* results from `probe astar`, parsed tables of both directions'
models from `probe hmm` (r600: the md5 of their bits).  r600 (tables beyond the LDS) keeps as many seeds as close no more nodes than bigm/m600_astar_cold;
r700 is eight seeds for the one lane mode in which 600 columns still fit the LDS."""
from __future__ import annotations

import hashlib
import json
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from megagta_amd import synth          # noqa: E402
from tests import helpers as H         # noqa: E402
from tests.golden.make_golden import run, gz_write, buildgraph, REF, GOLD   # noqa: E402
from tests.rich_models import RICHM_CASES as CASES, richm_inputs, tables_md5            # noqa: E402  (the tests regenerate the same inputs)


def closed_total(text: bytes) -> int:
    return sum(r["R"]["closed"] + r["L"]["closed"] for r in H.parse_probe_astar(text.decode().splitlines()))


def main():
    out = os.path.join(GOLD, "richm")
    shutil.rmtree(out, ignore_errors=True)
    os.makedirs(out)
    tmp = tempfile.mkdtemp(prefix="mgta_gold_richm_")
    budget = sum(r["R"]["closed"] + r["L"]["closed"] for r in H.parse_probe_astar(H.gz_lines(os.path.join(GOLD, "bigm", "m600_astar_cold.txt.gz"))))
    meta = {}
    for case, c in CASES.items():
        d = os.path.join(tmp, case)
        os.makedirs(d)
        mg, gdir = richm_inputs(case, d)
        synth.write_fasta(mg.reads, f"{d}/reads.fa")
        open(f"{d}/reads.lib", "w").write(f"reads.fa\nse {d}/reads.fa\n")
        run([f"{REF}/megagta", "buildlib", f"{d}/reads.lib", f"{d}/reads.lib"])
        buildgraph(f"{d}/reads.lib", f"{d}/k44/44", 44)
        found = sorted(run([f"{REF}/megagta", "findstart", f"{gdir}/ref_aligned.faa", f"{d}/reads.lib.bin", "45", "1"]).stdout.splitlines())
        n_seeds = c["n_seeds"]                             # (the reference shuffles its lines: sorted above)
        while True:
            seeds = found[::max(1, len(found) // n_seeds)][:n_seeds]
            open(f"{out}/{case}_starting_kmers.txt", "wb").write(b"\n".join(seeds) + b"\n")
            res = {}
            for mode in ("cold", "warm") if case == "r75" else ("cold",):
                res[mode] = run([f"{REF}/probe", "astar", f"{d}/k44/44", f"{gdir}/for_enone.hmm", f"{gdir}/rev_enone.hmm",
                                 f"{out}/{case}_starting_kmers.txt", str(c["prune"]), "0.5", mode]).stdout
            if case != "r600" or closed_total(res["cold"]) <= budget:
                break
            n_seeds -= 1                                   # thinned until the case costs no more than m600
            assert n_seeds > 0
        for mode, text in res.items():
            gz_write(f"{out}/{case}_astar_{mode}.txt.gz", text)
        tmd5 = {}
        for tag, name in (("for", "for_enone.hmm"), ("rev", "rev_enone.hmm")):
            tables = run([f"{REF}/probe", "hmm", f"{gdir}/{name}"]).stdout
            tmd5[tag] = tables_md5(H.parse_probe_hmm(tables.decode().splitlines()))
            if c["M"] < 400:                               # (r600, r700: 120 KB of tables per model; the md5 of their bits stands for them)
                gz_write(f"{out}/{case}_{tag}_tables.txt.gz", tables)
                shutil.copy(f"{gdir}/{name}", f"{out}/{case}_{name}")
        meta[case] = dict(c, n_seeds_found=len(found), n_seeds=len(seeds), closed_total=closed_total(res["cold"]), closed_total_m600=budget, tables_md5=tmd5,
                          md5={n: hashlib.md5(open(p, "rb").read()).hexdigest()
                               for n, p in (("reads", f"{d}/reads.lib.bin"), ("for", f"{gdir}/for_enone.hmm"), ("rev", f"{gdir}/rev_enone.hmm"))})
    json.dump(meta, open(f"{out}/cases.json", "w"), indent=1)
    shutil.rmtree(tmp)
    print("written", out, json.dumps(meta, indent=1))


if __name__ == "__main__":
    main()
