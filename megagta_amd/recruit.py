"""The files of `megagta recruit` / `megagta.py --recruit`: writers and readers, so that tests and users read them one way.  Host only,
no device.  The definitions are those of mgta_reads_recruit (include/megagta_hip.h, INTEGRATION.md 2h').

  recruit_reads.fa     `>r<i>` records of the recruited reads, exactly as matchreads.py writes a matched-reads file
  recruit.txt          #read<TAB>frame<TAB>aa_from<TAB>aa_len<TAB>bits<TAB>model_from<TAB>model_to, one line per recruited read,
                       ascending i; bits = score / ln 2 as %.4f; aa_from and aa_len as the record holds them: the scored stretch in
                       global mode, the aligned span in local mode
  recruit_cols.txt     #column<TAB>depth, one line per model column 1 .. M
  recruit_summary.txt  key<TAB>value lines: reads_scanned, reads_scored, reads_recruited, recruited_frame<f> (f = 0 .. 5),
                       recruited_lib<s> per library, in local mode (MGTA_RECRUIT_LOCAL) the line recruit_mode<TAB>local, and, when
                       the matched reads are known, recruited_and_matched and assembled_fraction (%.4f; 0.0000 when nothing is
                       recruited)
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib
from .matchreads import match_reads_text, parse_match_reads

LN2 = 0.6931471805599453          # the one constant bits are turned into nats with: nats = bits * LN2

REC = _lib.RECORDS[_lib.RecruitRec]                                   # mgta_recruit_rec
assert REC.itemsize == 24

HEADER = "#read\tframe\taa_from\taa_len\tbits\tmodel_from\tmodel_to"
COLS_HEADER = "#column\tdepth"


def hit_indices(hit_bits: np.ndarray, n_reads: int) -> np.ndarray:
    """the reads whose bit is on, ascending (bit r of word r // 64)"""
    bits = np.unpackbits(np.ascontiguousarray(hit_bits, dtype="<u8").view(np.uint8), bitorder="little")[:n_reads]
    return np.flatnonzero(bits).astype(np.int64)


def lib_counts(hit_bits: np.ndarray, lib_end) -> list[int]:
    """recruited reads per library: the bits on in [lib_end[s - 1], lib_end[s])"""
    ends = [int(e) for e in lib_end]
    idx = hit_indices(hit_bits, ends[-1] if ends else 0)
    cuts = np.searchsorted(idx, [0] + ends)
    return [int(cuts[s + 1] - cuts[s]) for s in range(len(ends))]


def recruit_text(recs: np.ndarray, idx) -> str:
    """the text of recruit.txt for the recruited reads idx"""
    lines = [HEADER]
    for i in np.sort(np.asarray(idx, dtype=np.int64)):
        r = recs[int(i)]
        lines.append("%d\t%d\t%d\t%d\t%.4f\t%d\t%d" % (i, r["frame"], r["aa_from"], r["aa_len"], float(r["score"]) / math.log(2.0), r["model_from"], r["model_to"]))
    return "\n".join(lines) + "\n"


def parse_recruit(text: str) -> list[dict]:
    lines = text.splitlines()
    if not lines or lines[0] != HEADER:
        raise ValueError("recruit text: the header line is missing")
    out = []
    for ln in lines[1:]:
        f = ln.split("\t")
        if len(f) != 7:
            raise ValueError(f"recruit text: bad line {ln!r}")
        out.append(dict(read=int(f[0]), frame=int(f[1]), aa_from=int(f[2]), aa_len=int(f[3]), bits=float(f[4]), model_from=int(f[5]), model_to=int(f[6])))
    return out


def cols_text(col_depth) -> str:
    return COLS_HEADER + "\n" + "".join("%d\t%d\n" % (j + 1, int(d)) for j, d in enumerate(col_depth))


def parse_cols(text: str) -> np.ndarray:
    lines = text.splitlines()
    if not lines or lines[0] != COLS_HEADER:
        raise ValueError("recruit columns text: the header line is missing")
    depth = []
    for j, ln in enumerate(lines[1:]):
        f = ln.split("\t")
        if len(f) != 2 or int(f[0]) != j + 1:
            raise ValueError(f"recruit columns text: bad line {ln!r}")
        depth.append(int(f[1]))
    return np.array(depth, dtype=np.uint64)


def assembled_fraction(recruited, matched) -> tuple[int, float]:
    """(reads in both index sets, their share of the recruited ones; 0.0 when none is recruited)"""
    rec = np.unique(np.asarray(recruited, dtype=np.int64))
    both = int(np.intersect1d(rec, np.asarray(matched, dtype=np.int64)).size)
    return both, (both / rec.size if rec.size else 0.0)


def summary_text(stats: dict, per_lib=None, recruited=None, matched=None, local: bool = False) -> str:
    """the text of recruit_summary.txt from the stats of Context.recruit; per_lib = lib_counts(...) of a run with libraries;
    recruited and matched = the two index sets when --match-reads was part of the run; local = the run was made in local mode"""
    lines = ["reads_scanned\t%d" % stats["n_reads"], "reads_scored\t%d" % (stats["n_reads"] - stats["n_unscored"]), "reads_recruited\t%d" % stats["n_recruited"]]
    lines += ["recruited_frame%d\t%d" % (f, int(c)) for f, c in enumerate(stats["n_recruited_frame"])]
    if per_lib is not None:
        lines += ["recruited_lib%d\t%d" % (s, int(c)) for s, c in enumerate(per_lib)]
    if local:
        lines.append("recruit_mode\tlocal")
    if matched is not None:
        both, frac = assembled_fraction(recruited, matched)
        lines += ["recruited_and_matched\t%d" % both, "assembled_fraction\t%.4f" % frac]
    return "\n".join(lines) + "\n"


def parse_summary(text: str) -> dict:
    out = {}
    for ln in text.splitlines():
        key, _, val = ln.partition("\t")
        if not key or not val:
            raise ValueError(f"recruit summary text: bad line {ln!r}")
        out[key] = val if key == "recruit_mode" else float(val) if key == "assembled_fraction" else int(val)
    return out


def append_assembled(summary_path: str, recruit_fa: str, match_fa: str) -> tuple[int, float]:
    """recruited_and_matched and assembled_fraction behind the lines of a summary file, from the two read files of a gene (lines of
    those names that are there already are replaced) -> (reads in both, their share of the recruited)"""
    def indices(path):
        with open(path) as fh:
            return parse_match_reads(fh.read())[0]
    both, frac = assembled_fraction(indices(recruit_fa), indices(match_fa))
    with open(summary_path) as fh:
        lines = [ln for ln in fh.read().splitlines() if ln.partition("\t")[0] not in ("recruited_and_matched", "assembled_fraction")]
    lines += ["recruited_and_matched\t%d" % both, "assembled_fraction\t%.4f" % frac]
    with open(summary_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return both, frac


def write_files(out_dir: str, res: dict, packed: np.ndarray, start: np.ndarray, lib_end=None, matched=None, reversed_storage: bool = True,
                local: bool = False) -> dict:
    """the four files of a gene under out_dir from res = Context.recruit(..., recs=True, cols=True); local = it ran in local mode;
    -> their paths"""
    import os
    n = int(res["stats"]["n_reads"])
    idx = hit_indices(res["hit_bits"], n)
    paths = {name: os.path.join(out_dir, name) for name in ("recruit_reads.fa", "recruit.txt", "recruit_cols.txt", "recruit_summary.txt")}
    texts = {"recruit_reads.fa": match_reads_text(idx, packed, start, reversed_storage), "recruit.txt": recruit_text(res["recs"], idx),
             "recruit_cols.txt": cols_text(res["col_depth"]),
             "recruit_summary.txt": summary_text(res["stats"], lib_counts(res["hit_bits"], lib_end) if lib_end is not None else None, idx, matched, local)}
    for name, text in texts.items():
        with open(paths[name], "w") as fh:
            fh.write(text)
    return paths


def read_files(out_dir: str) -> dict:
    import os
    def text(name):
        with open(os.path.join(out_dir, name)) as fh:
            return fh.read()
    idx, seqs = parse_match_reads(text("recruit_reads.fa"))
    return dict(reads=idx, seqs=seqs, recs=parse_recruit(text("recruit.txt")), col_depth=parse_cols(text("recruit_cols.txt")), summary=parse_summary(text("recruit_summary.txt")))
