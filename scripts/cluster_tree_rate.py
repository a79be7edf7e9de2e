#!/usr/bin/env python3
"""The merge tree on the device (mgta_pairs_tree + mgta_tree_cut) next to the host linkage (mgta_pairs_link) on the same pair list, in
one process, on the input of scripts/cluster_rate.py.

python scripts/cluster_tree_rate.py [--rows 20000] [--cols 300] [--span 150] [--cutoffs 0.01,0.05] [--min-overlap 25] [--repeat 3]
                                    [--three 0.01,0.03,0.05] [--out profiles/cluster/run_tree.json]

Per cut-off D of `--cutoffs`: the kept pairs at D once (Context.row_pairs), then, each after one warm-up call and as the best of
`repeat` calls, Context.pairs_tree on them (ms_build, ms_rounds: HIP events of the library; wall), api.tree_cut at D (ms_cut) and
api.link_pairs (ms_link, the host linkage's own clock); the clusters of the two routes are compared row for row.  Printed with them:
n_rounds, n_entries_visited / (2 n_pairs), n_lists_rewritten, the kept pairs and the peak device memory of the tree call.
`--three`: the wall time of one Context.clusters call at those cut-offs against three Context.cluster calls."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from megagta_amd import api  # noqa: E402
from cluster_rate import GAP, make_rows  # noqa: E402


def best_of(repeat, call):
    call()                                                                # the warm-up
    runs = []
    for _ in range(repeat):
        t0 = time.time()
        res = call()
        runs.append((time.time() - t0, res))
    return runs


def main(argv):
    opt = {"--rows": "20000", "--cols": "300", "--span": "150", "--cutoffs": "0.01,0.05", "--min-overlap": "25", "--repeat": "3", "--three": "0.01,0.03,0.05", "--out": ""}
    for a, v in zip(argv[0::2], argv[1::2]):
        if a not in opt:
            raise SystemExit(__doc__)
        opt[a] = v
    n, M, min_overlap, repeat = int(opt["--rows"]), int(opt["--cols"]), int(opt["--min-overlap"]), int(opt["--repeat"])
    rows = make_rows(n, M, int(opt["--span"]))
    lens = (rows != GAP).sum(axis=1)
    n_res = lens.astype(np.int32)
    ctx = api.Context(0)
    line = dict(rows=n, cols=M, span=int(opt["--span"]), min_overlap=min_overlap, repeat=repeat, cutoffs=[])
    for D in [float(x) for x in opt["--cutoffs"].split(",") if x]:
        pairs = ctx.row_pairs(rows, min_overlap, D)["pairs"]
        trees = best_of(repeat, lambda: ctx.pairs_tree(pairs, n_res))
        tree = trees[0][1]
        cuts = best_of(repeat, lambda: api.tree_cut(pairs, tree["merges"], n_res, lens, D))
        links = best_of(repeat, lambda: api.link_pairs(pairs, n_res, lens))
        cut, link = cuts[0][1], links[0][1]
        same = all(np.array_equal(cut[f], link[f]) for f in ("cluster", "rep", "rep_diff", "rep_overlap"))
        st = tree["stats"]
        line["cutoffs"].append(dict(
            cutoff=D, n_pairs=int(len(pairs)), n_merges=int(st["n_merges"]), n_rounds=int(st["n_rounds"]), n_lists_rewritten=int(st["n_lists_rewritten"]),
            n_entries_visited=int(st["n_entries_visited"]), visits_per_entry=st["n_entries_visited"] / (2 * len(pairs)) if len(pairs) else None,
            peak_device_bytes=int(st["peak_bytes"]), ms_build=min(r["stats"]["ms_build"] for _, r in trees), ms_rounds=min(r["stats"]["ms_rounds"] for _, r in trees),
            ms_tree_wall=1e3 * min(t for t, _ in trees), ms_cut=min(r["stats"]["ms_cut"] for _, r in cuts), ms_link=min(r["stats"]["ms_link"] for _, r in links),
            ms_link_wall=1e3 * min(t for t, _ in links), n_cut_fallbacks=int(cut["stats"]["n_cut_fallbacks"]), n_clusters=int(cut["stats"]["n_clusters"]),
            clusters_equal=bool(same)))
        print(json.dumps(line["cutoffs"][-1]), flush=True)
        assert same, "the cut of the tree and the host linkage disagree"
    three = [float(x) for x in opt["--three"].split(",") if x]
    if three:
        one = best_of(repeat, lambda: ctx.clusters(rows, lens, min_overlap, three))
        each = best_of(repeat, lambda: [ctx.cluster(rows, lens, min_overlap, c) for c in three])
        same = all(np.array_equal(one[0][1]["cluster"][k], each[0][1][k]["cluster"]) for k in range(len(three)))
        st = one[0][1]["stats"]
        line["three"] = dict(cutoffs=three, s_one_tree=min(t for t, _ in one), s_separate_calls=min(t for t, _ in each), clusters_equal=bool(same),
                             ms_pairs=st["ms_pairs"], ms_build=st["ms_build"], ms_rounds=st["ms_rounds"], ms_cut=st["ms_cut"], n_pairs=int(st["n_pairs"]),
                             n_rounds=int(st["n_rounds"]), peak_device_bytes=int(st["peak_bytes"]))
        print(json.dumps(line["three"]), flush=True)
        assert same, "Context.clusters and Context.cluster disagree"
    print(json.dumps(line), flush=True)
    if opt["--out"]:
        with open(opt["--out"], "w") as fh:
            fh.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1:])
