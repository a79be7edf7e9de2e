#!/usr/bin/env python3
"""The rate of mgta_seqs_derep on a synthetic gene's worth of contigs.

python scripts/derep_rate.py [--seqs 1000000] [--parents 200] [--parent-len 280] [--host-seconds 60] [--out profiles/derep/run.json]

The input is the generator of tests/test_derep_gpu.py scaled up: `parents` random protein sequences of `parent-len` letters and, per
sequence, a random piece of a parent of 150 letters or more (the product's contigs are at least that long), one in ten with one letter
changed (a variant of its own: kept unless a copy exists), one in ten an exact copy of an earlier sequence.  Printed per size: letters
per second over the three timed parts, the parts themselves (HIP events of the library), n_compares / n_first -- if that grows with
the input at a fixed parent count the anchor choice is not doing its job -- and the device bytes of the call's buffers at their peak,
summed from the sizes the library allocates (documented in include/megagta_hip.h; the library does not report its peak).

Beside it the time of a plain host implementation of the same rule, in this script and not in the product: a set for the duplicates
and a substring search over the longer distinct sequences, longest first, on as many sequences as finish in `host-seconds`."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from megagta_amd import api  # noqa: E402

AA = np.frombuffer(b"acdefghiklmnpqrstvwy", dtype=np.uint8)


def make_contigs(n: int, parents: int, parent_len: int, seed: int = 7) -> list[bytes]:
    rng = np.random.default_rng(seed)
    par = AA[rng.integers(0, 20, (parents, parent_len))]
    which = rng.integers(0, parents, n)
    lens = rng.integers(min(150, parent_len), parent_len + 1, n)
    starts = (rng.random(n) * (parent_len - lens + 1)).astype(np.int64)
    kind = rng.integers(0, 10, n)                                        # 0: one letter changed, 1: a copy of an earlier one
    at = (rng.random(n) * lens).astype(np.int64)
    other = AA[rng.integers(0, 20, n)]
    src = (rng.random(n) * np.arange(n)).astype(np.int64)
    out = []
    for i in range(n):
        if kind[i] == 1 and i:
            out.append(out[src[i]])
            continue
        s = par[which[i], starts[i]:starts[i] + lens[i]]
        if kind[i] == 0:
            s = s.copy()
            s[at[i]] = other[i]
        out.append(s.tobytes())
    return out


def host_derep(seqs: list[bytes]) -> tuple[int, int, int]:
    """the rule on the host -> (kept, duplicate, contained)"""
    first = {}
    for i, s in enumerate(seqs):
        first.setdefault(s, i)
    distinct = sorted(first, key=len, reverse=True)
    contained = 0
    for j, s in enumerate(distinct):
        n = len(s)
        for t in distinct[:j]:
            if len(t) == n:
                break
            if s in t:
                contained += 1
                break
    return len(distinct) - contained, len(seqs) - len(distinct), contained


def peak_bytes(st: dict) -> int:
    n, a = st["n_seqs"], st["anchor_len"]
    dup_slots = 64
    while dup_slots < 2 * n:
        dup_slots *= 2
    phase1 = st["n_letters"] + 8 * (n + 1) + 8 * n + 8 * n + 8 * dup_slots + 4 * n
    first_letters = st["n_windows"] + st["n_first"] * max(0, a - 1)
    win_slots = 64
    while win_slots < 2 * st["n_windows"]:
        win_slots *= 2
    phase2 = 9 * first_letters + 16 * win_slots + 17 * st["n_first"]
    return max(phase1, phase2)


def one_size(ctx, n: int, parents: int, parent_len: int) -> dict:
    seqs = make_contigs(n, parents, parent_len)
    ctx.derep(seqs[:1000])                                               # warm: the code object
    t0 = time.time()
    st = ctx.derep(seqs)["stats"]
    wall = time.time() - t0
    ms = st["ms_dups"] + st["ms_table"] + st["ms_verify"]
    return dict(seqs=n, parents=parents, parent_len=parent_len, stats=st, letters_per_s=st["n_letters"] / (ms * 1e-3), ms_device=ms, wall_s=wall,
                compares_per_first=st["n_compares"] / max(1, st["n_first"]), peak_device_bytes=peak_bytes(st))


def host_baseline(parents: int, parent_len: int, budget_s: float) -> dict:
    n, last = 2000, None
    while True:
        seqs = make_contigs(n, parents, parent_len)
        t0 = time.time()
        kept, dup, cont = host_derep(seqs)
        dt = time.time() - t0
        last = dict(seqs=n, letters=sum(map(len, seqs)), seconds=dt, kept=kept, duplicate=dup, contained=cont)
        if dt * 4 > budget_s:                                            # (the next size would take about four times as long)
            return last
        n *= 2


def main(argv):
    sizes, parents, parent_len, host_s, out_path = [1_000_000], 200, 280, 60.0, None
    it = iter(argv)
    for a in it:
        if a == "--seqs":
            sizes = [int(x) for x in next(it).split(",")]
        elif a == "--parents":
            parents = int(next(it))
        elif a == "--parent-len":
            parent_len = int(next(it))
        elif a == "--host-seconds":
            host_s = float(next(it))
        elif a == "--out":
            out_path = next(it)
        else:
            print(__doc__)
            return 2
    ctx = api.Context(0)
    res = {"sizes": []}
    for n in sizes:
        res["sizes"].append(one_size(ctx, n, parents, parent_len))
        print(json.dumps(res["sizes"][-1]), flush=True)
    ctx.close()
    res["host"] = host_baseline(parents, parent_len, host_s) if host_s > 0 else None
    print(json.dumps({"host": res["host"]}), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
