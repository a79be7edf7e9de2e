#!/usr/bin/env python3
"""The rate of mgta_reads_match_contigs (the read walk) against the device's pointer-chase rate.

python scripts/matchreads_rate.py [--reads 1000000,10000000] [--k 44] [--out profiles/matchreads/run.json]

For every size: the bench's synthetic reads (synth.make_metagenome_device, 150 bp, one gene) are drawn on the device, their `-m 1` graph
is built and loaded where it lies, and the reads are matched against the contigs of the gene -- its copies in the sample's genomes,
the sequences the search assembles -- once with bits only (a read's walk ends at its first hit) and once with counts (every window
is walked).  Printed and written: read windows per second and microseconds per visited window per lane group from the library's HIP
events, and beside it, from the same process, mgta_probe_random_lines with dependent = 1 at the kernel's own shape (8 groups per
wave, stats.groups_per_cu / 8 waves per CU) -- one dependent line per window is the floor of the design, so
"x of the chase rate" = (probe ns per step) / (walk ns per visited window per group)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before the first call into the library: one HIP runtime serves both)

from megagta_amd import api, synth  # noqa: E402

DNA = "ACGT"


def one_size(ctx, n_reads: int, k: int, cus: int) -> dict:
    mg = synth.make_metagenome_device(n_reads, 150, (("rplB", 277),), seed=1000 + n_reads % 997, host_sample=0)
    rd = ctx.adopt_reads(mg.packed.data_ptr(), mg.n_words, mg.start.data_ptr(), mg.n_reads, keepalive=(mg.packed, mg.start))
    build = ctx.build_sdbg(rd, k, collect=False).stats
    g = api.Graph(ctx, None)
    contigs = ["".join(DNA[c] for c in v) for v in mg.genes[0].variants]
    g.match_reads(rd, contigs, n_short_reads=min(n_reads, 100000))         # warm: the marks, the code object
    out = dict(reads=n_reads, k=k, edges=g.size, contigs=len(contigs), build_passes=build["n_passes"], runs={})
    for name, counts in (("bits_only", False), ("counts", True)):
        st = g.match_reads(rd, contigs, counts=counts)["stats"]
        visited = st["n_walked"] + st["n_index_searches"]
        groups = min(cus * st["groups_per_cu"], n_reads)
        out["runs"][name] = dict(stats=st, visited_windows=visited, read_windows_per_s=st["n_read_windows"] / (st["ms_walk"] * 1e-3),
                                 visited_windows_per_s=visited / (st["ms_walk"] * 1e-3), index_search_share=st["n_index_searches"] / max(1, visited),
                                 us_per_visited_window_per_group=st["ms_walk"] * 1e3 * groups / max(1, visited), groups=groups)
    g.free()
    rd.free()
    ctx.release_scratch()
    del mg
    torch.cuda.empty_cache()
    return out


def main(argv):
    sizes, k, out_path = [1_000_000, 10_000_000], 44, None
    it = iter(argv)
    for a in it:
        if a == "--reads":
            sizes = [int(x) for x in next(it).split(",")]
        elif a == "--k":
            k = int(next(it))
        elif a == "--out":
            out_path = next(it)
        else:
            print(__doc__)
            return 2
    ctx = api.Context(0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    res = {"sizes": [one_size(ctx, n, k, cus) for n in sizes]}
    gpc = res["sizes"][0]["runs"]["counts"]["stats"]["groups_per_cu"]
    waves = max(1, min(32, gpc // 8))
    probe = ctx.probe_random_lines(16 << 30, [(waves, 8, 1, 1, 20000)])[0]
    res["probe_dependent"] = probe
    for s in res["sizes"]:
        for r in s["runs"].values():
            r["of_chase_rate"] = probe["ns_per_step"] * 1e-3 / r["us_per_visited_window_per_group"]
    text = json.dumps(res, indent=1)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
