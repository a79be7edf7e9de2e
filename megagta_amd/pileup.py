"""Pileup files: what `megagta.py --pileup` writes from Graph.pileup (mgta_reads_pileup, include/megagta_hip.h).

  PREFIX_pileup.txt           `#contig len reads unique covered min max mean mismatches variants` (tabs), then one line per FASTA
                              record in file order.  reads = placements on the contig, unique = those of reads placed once, covered =
                              positions with depth > 0, mean = floor(depth_sum * 10000 / len) printed with four decimals (0.0000 for
                              len 0), mismatches = the sum of the placements' mismatches, variants = the contig's lines in the next file.
  PREFIX_pileup_variants.txt  `#contig pos ref depth A C G T unique`: pos is 1-based, ref the contig's letter as given.  A position is
                              listed iff depth >= min_depth (default 8) and alt * 1000 >= min_alt_permille * depth (default 100), with
                              alt = depth - counts[ref folded to upper case], alt = depth where ref is none of A C G T.
  PREFIX_pileup_depth.txt     the same columns for every position (`--per-base`).

The rule of the placements is the library's; this module holds the variant rule and the writers and readers of the three files.
"""
from __future__ import annotations

import numpy as np

from . import _lib

CONTIG_DTYPE = _lib.RECORDS[_lib.ContigPileup]                        # mgta_contig_pileup
READ_DTYPE = _lib.RECORDS[_lib.ReadPlace]                             # mgta_read_place
SUMMARY_HEADER = "#contig\tlen\treads\tunique\tcovered\tmin\tmax\tmean\tmismatches\tvariants\n"
BASE_HEADER = "#contig\tpos\tref\tdepth\tA\tC\tG\tT\tunique\n"
MIN_DEPTH, MIN_ALT_PERMILLE = 8, 100
_BASES = "ACGT"


def _text(s) -> str:
    return s.decode() if isinstance(s, (bytes, bytearray)) else str(s)


def variant_mask(seq, counts, min_depth: int = MIN_DEPTH, min_alt_permille: int = MIN_ALT_PERMILLE) -> np.ndarray:
    """bool[len]: the positions of one contig that are listed.  counts = its rows [len, 4]"""
    seq = _text(seq).upper()
    c = np.asarray(counts, dtype=np.int64).reshape(len(seq), 4)
    depth = c.sum(axis=1)
    ref = np.array([_BASES.find(ch) for ch in seq], dtype=np.int64)
    own = np.where(ref >= 0, c[np.arange(len(seq)), np.maximum(ref, 0)], 0) if len(seq) else np.zeros(0, dtype=np.int64)
    alt = depth - own
    return (depth >= int(min_depth)) & (alt * 1000 >= int(min_alt_permille) * depth)


def _base_lines(name: str, seq: str, counts, uniq, which) -> list[str]:
    out = []
    for x in which:
        a, c, g, t = (int(v) for v in counts[x])
        out.append(f"{name}\t{x + 1}\t{seq[x]}\t{a + c + g + t}\t{a}\t{c}\t{g}\t{t}\t{int(uniq[x])}\n")
    return out


def format_pileup(names, seqs, res, min_depth: int = MIN_DEPTH, min_alt_permille: int = MIN_ALT_PERMILLE, per_base: bool = False) -> dict:
    """names and letters of the FASTA records in file order + the dict Graph.pileup returned for them -> dict(summary=, variants=,
    depth= (None without per_base)): the texts of the three files"""
    rec, counts, uniq, off = res["contigs"], res["counts"], res["uniq"], res["offsets"]
    if not (len(names) == len(seqs) == len(rec)):
        raise ValueError("names, sequences and records differ in number")
    summary, variants, depth = [SUMMARY_HEADER], [BASE_HEADER], [BASE_HEADER]
    for i, (name, seq) in enumerate(zip(names, seqs)):
        seq = _text(seq)
        if int(off[i + 1] - off[i]) != len(seq) or int(rec[i]["len"]) != len(seq):
            raise ValueError(f"record {i}: the result was computed for other sequences")
        c, u = counts[int(off[i]):int(off[i + 1])], uniq[int(off[i]):int(off[i + 1])]
        listed = np.flatnonzero(variant_mask(seq, c, min_depth, min_alt_permille))
        variants += _base_lines(name, seq, c, u, listed)
        if per_base:
            depth += _base_lines(name, seq, c, u, range(len(seq)))
        r = rec[i]
        mean = int(r["depth_sum"]) * 10000 // len(seq) if len(seq) else 0
        summary.append(f"{name}\t{len(seq)}\t{int(r['n_placed'])}\t{int(r['n_unique'])}\t{int(r['n_covered'])}\t{int(r['min_depth'])}\t{int(r['max_depth'])}\t"
                       f"{mean // 10000}.{mean % 10000:04d}\t{int(r['mismatch_sum'])}\t{len(listed)}\n")
    return dict(summary="".join(summary), variants="".join(variants), depth="".join(depth) if per_base else None)


def write_pileup(prefix: str, names, seqs, res, min_depth: int = MIN_DEPTH, min_alt_permille: int = MIN_ALT_PERMILLE, per_base: bool = False) -> list[str]:
    """-> the paths written"""
    texts = format_pileup(names, seqs, res, min_depth, min_alt_permille, per_base)
    paths = []
    for key, suffix in (("summary", "_pileup.txt"), ("variants", "_pileup_variants.txt"), ("depth", "_pileup_depth.txt")):
        if texts[key] is not None:
            with open(prefix + suffix, "w") as f:
                f.write(texts[key])
            paths.append(prefix + suffix)
    return paths


def parse_summary(text: str) -> list[dict]:
    lines = text.splitlines(keepends=True)
    if not lines or lines[0] != SUMMARY_HEADER:
        raise ValueError("not a pileup summary: the header line differs")
    out = []
    for ln in lines[1:]:
        f = ln.rstrip("\n").split("\t")
        if len(f) != 10:
            raise ValueError(f"pileup summary: {len(f)} fields in {ln!r}")
        whole, frac = f[7].split(".")
        if len(frac) != 4:
            raise ValueError(f"pileup summary: the mean {f[7]!r} has not four decimals")
        out.append(dict(contig=f[0], len=int(f[1]), reads=int(f[2]), unique=int(f[3]), covered=int(f[4]), min=int(f[5]), max=int(f[6]),
                        mean_e4=int(whole) * 10000 + int(frac), mismatches=int(f[8]), variants=int(f[9])))
    return out


def parse_bases(text: str) -> list[dict]:
    """the lines of a variants or a depth file"""
    lines = text.splitlines(keepends=True)
    if not lines or lines[0] != BASE_HEADER:
        raise ValueError("not a pileup position file: the header line differs")
    out = []
    for ln in lines[1:]:
        f = ln.rstrip("\n").split("\t")
        if len(f) != 9:
            raise ValueError(f"pileup positions: {len(f)} fields in {ln!r}")
        row = dict(contig=f[0], pos=int(f[1]), ref=f[2], depth=int(f[3]), A=int(f[4]), C=int(f[5]), G=int(f[6]), T=int(f[7]), unique=int(f[8]))
        if row["depth"] != row["A"] + row["C"] + row["G"] + row["T"]:
            raise ValueError(f"pileup positions: depth is not A + C + G + T in {ln!r}")
        out.append(row)
    return out


def read_fasta(path: str) -> tuple[list[str], list[str]]:
    """names (the header up to its first blank) and letters of a FASTA file, in file order"""
    names, seqs = [], []
    with open(path) as f:
        for ln in f:
            ln = ln.rstrip("\r\n").rstrip(" \t")
            if ln.startswith(">"):
                names.append(ln[1:].replace("\t", " ").split(" ")[0])
                seqs.append([])
            elif seqs:
                seqs[-1].append(ln.lstrip(" \t"))
    return names, ["".join(s) for s in seqs]
