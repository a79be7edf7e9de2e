#!/usr/bin/env python3
"""The rate of mgta_contig_coverage against the device's pointer-chase rate, and what the opt-in multiplicities cost in memory.

python scripts/coverage_rate.py <sdbg_prefix> <contigs.fasta> [more.fasta ...] [--out profiles/coverage/run.json]

<sdbg_prefix>: the graph files of a finished run's last k (out/k44/44); the FASTA files: contigs/<gene>/nucl_merged.fasta of its genes.
Prints and writes: windows per second and microseconds per window per lane group from the library's HIP events, the share of windows
that needed an index search, and beside it, from the same process, mgta_probe_random_lines with dependent = 1 at the kernel's own
shape (8 groups per wave, as many waves per CU as the walk kernel holds: stats.groups_per_cu / 8, which the library asks of the
runtime) -- one dependent line per window is the floor of the design, so
"x of the chase rate" = (probe ns per step) / (walk ns per window per group).  Device memory free before / after a load with the
switch off and on (mgta_ctx_device_memory) gives the measured cost of the multiplicities."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ctypes as C  # noqa: E402

from megagta_amd import api, coverage as cv  # noqa: E402


def free_bytes(ctx):
    f, t = C.c_uint64(), C.c_uint64()
    api.check(ctx._L.mgta_ctx_device_memory(ctx.h, C.byref(f), C.byref(t)), "mgta_ctx_device_memory")
    return f.value


def main(argv):
    out_path = None
    if "--out" in argv:
        i = argv.index("--out")
        out_path = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    if len(argv) < 2:
        print(__doc__)
        return 2
    prefix, fastas = argv[0], argv[1:]
    ctx = api.Context(0)
    res = {"sdbg_prefix": prefix, "fastas": fastas}
    f0 = free_bytes(ctx)
    g = api.Graph.from_files(ctx, prefix)
    f1 = free_bytes(ctx)
    g.free()
    t = time.time()
    g = api.Graph.from_files(ctx, prefix, keep_multiplicity=True)
    res["load_with_multiplicity_s"] = time.time() - t
    f2 = free_bytes(ctx)
    res.update(edges=g.size, k=g.k, graph_bytes_switch_off=f0 - f1, graph_bytes_switch_on=f0 - f2,
               multiplicity_bytes_per_edge=(f1 - f2) / max(1, g.size))
    import torch                            # (only for the CU count)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    runs = []
    for fa in fastas:
        names, seqs = cv.read_fasta(fa)
        g.contig_coverage(seqs[:1000])      # warm: scratch, marks
        t = time.time()
        r = g.contig_coverage(seqs)
        wall = time.time() - t
        st = r["stats"]
        groups = min(cus * st["groups_per_cu"], len(seqs))
        runs.append(dict(fasta=fa, contigs=len(seqs), windows=st["n_windows"], index_search_share=st["n_index_searches"] / max(1, st["n_windows"]),
                         ms_walk=st["ms_walk"], ms_kernel=st["ms_kernel"], wall_s=wall, windows_per_s=st["n_windows"] / (st["ms_walk"] * 1e-3),
                         us_per_window_per_group=st["ms_walk"] * 1e3 * groups / max(1, st["n_windows"]), groups=groups, groups_per_cu=st["groups_per_cu"],
                         batches=st["n_batches"]))
    res["coverage"] = runs
    waves = max(1, min(32, runs[0]["groups_per_cu"] // 8))
    probe = ctx.probe_random_lines(16 << 30, [(waves, 8, 1, 1, 20000)])[0]
    res["probe_dependent"] = probe
    for r in runs:
        r["of_chase_rate"] = probe["ns_per_step"] * 1e-3 / r["us_per_window_per_group"]
    text = json.dumps(res, indent=1)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
