"""Gapped pileup files: what `megagta.py --pileup --gapped` writes from Graph.pileup_gapped (mgta_reads_pileup_gapped,
include/megagta_hip.h, INTEGRATION.md 2p').

  PREFIX_pileup.txt, PREFIX_pileup_variants.txt, PREFIX_pileup_depth.txt   as pileup.py writes them, from the gapped counts.
  PREFIX_pileup_indels.txt   `#contig pos type len seq reads unique depth` (tabs).  One line per event = the gap records that agree in
                             (contig, pos, type, len, letters).  pos is 1-based: the first deleted letter, or the letter in front of
                             which the insertion lies.  type = `del` or `ins`; seq = the deleted letters of the contig as given, or the
                             inserted letters of the read in the contig's strand; reads = the gapped placements that carry the event,
                             unique = those of reads placed once; depth = A + C + G + T of the counts at pos.  An event is listed iff
                             reads >= min_depth * min_alt_permille / 1000, rounded up, and at least 1.  Lines are ordered by contig (file
                             order), pos, insertions before deletions, len, seq.

The rule of the placements is the library's; this module holds the event rule, the listing rule, the writer and the readers, and
as_read_place(), which hands the per-read records on to Context.phase (a gapped placement gives no allele: n_placed = 0).
"""
from __future__ import annotations

import sys

import numpy as np

from . import _lib
from .pileup import MIN_ALT_PERMILLE, MIN_DEPTH, READ_DTYPE, _text, format_pileup

PLACE_DTYPE = _lib.RECORDS[_lib.GapPlace]                             # mgta_gap_place
GAP_DTYPE = _lib.RECORDS[_lib.GapRec]                                 # mgta_gap_rec
INDEL_HEADER = "#contig\tpos\ttype\tlen\tseq\treads\tunique\tdepth\n"
_BASES = "ACGT"
_COMP = str.maketrans("ACGT", "TGCA")


def read_letters(read, orient: int) -> str:
    """a read as sequenced (str, or an array of base codes 0..3) -> its letters in orientation `orient`"""
    s = read if isinstance(read, str) else "".join(_BASES[int(c)] for c in read)
    return s.translate(_COMP)[::-1] if orient else s


def events(gaps, seqs, reads, counts, offsets) -> list[dict]:
    """the gap records of one call -> its events in file order: dict(contig (index), pos (0-based), type, len, seq, reads, unique, depth).
    seqs = the contigs of the call, reads = the reads as sequenced (indexable by read number: str or base codes), counts and offsets =
    those of the call's result"""
    found = {}
    for g in gaps:
        i, pos, ln = int(g["contig"]), int(g["pos"]), int(g["len"])
        if ln > 0:
            letters = _text(seqs[i])[pos:pos + ln]
        else:
            letters = read_letters(reads[int(g["read"])], int(g["orient"]))[int(g["brk"]):int(g["brk"]) - ln]
        e = found.setdefault((i, pos, ln > 0, abs(ln), letters), [0, 0])
        e[0] += 1
        e[1] += int(g["unique"]) != 0
    out = []
    for (i, pos, is_del, ln, letters), (n, u) in sorted(found.items()):
        depth = int(np.asarray(counts[int(offsets[i]) + pos], dtype=np.int64).sum())
        out.append(dict(contig=i, pos=pos, type="del" if is_del else "ins", len=ln, seq=letters, reads=n, unique=u, depth=depth))
    return out


def min_reads(min_depth: int = MIN_DEPTH, min_alt_permille: int = MIN_ALT_PERMILLE) -> int:
    """the fewest reads of a listed event"""
    return max(1, (int(min_depth) * int(min_alt_permille) + 999) // 1000)


def format_indels(names, evs, min_depth: int = MIN_DEPTH, min_alt_permille: int = MIN_ALT_PERMILLE) -> str:
    """the text of PREFIX_pileup_indels.txt"""
    need = min_reads(min_depth, min_alt_permille)
    out = [INDEL_HEADER]
    for e in evs:
        if e["reads"] >= need:
            out.append(f"{names[e['contig']]}\t{e['pos'] + 1}\t{e['type']}\t{e['len']}\t{e['seq']}\t{e['reads']}\t{e['unique']}\t{e['depth']}\n")
    return "".join(out)


def format_gapped(names, seqs, res, reads, min_depth: int = MIN_DEPTH, min_alt_permille: int = MIN_ALT_PERMILLE, per_base: bool = False) -> dict:
    """pileup.format_pileup on the gapped result, and indels = the text of the fourth file"""
    texts = format_pileup(names, seqs, res, min_depth, min_alt_permille, per_base)
    texts["indels"] = format_indels(names, events(res["gaps"], seqs, reads, res["counts"], res["offsets"]), min_depth, min_alt_permille)
    return texts


def write_gapped(prefix: str, names, seqs, res, reads, min_depth: int = MIN_DEPTH, min_alt_permille: int = MIN_ALT_PERMILLE, per_base: bool = False) -> list[str]:
    """-> the paths written"""
    texts = format_gapped(names, seqs, res, reads, min_depth, min_alt_permille, per_base)
    paths = []
    for key, suffix in (("summary", "_pileup.txt"), ("variants", "_pileup_variants.txt"), ("depth", "_pileup_depth.txt"), ("indels", "_pileup_indels.txt")):
        if texts[key] is not None:
            with open(prefix + suffix, "w") as f:
                f.write(texts[key])
            paths.append(prefix + suffix)
    return paths


def parse_indels(text: str) -> list[dict]:
    lines = text.splitlines(keepends=True)
    if not lines or lines[0] != INDEL_HEADER:
        raise ValueError("not a pileup indel file: the header line differs")
    out = []
    for ln in lines[1:]:
        f = ln.rstrip("\n").split("\t")
        if len(f) != 8 or f[2] not in ("del", "ins"):
            raise ValueError(f"pileup indels: bad line {ln!r}")
        row = dict(contig=f[0], pos=int(f[1]), type=f[2], len=int(f[3]), seq=f[4], reads=int(f[5]), unique=int(f[6]), depth=int(f[7]))
        if row["len"] != len(row["seq"]) or row["len"] < 1 or row["unique"] > row["reads"] or row["reads"] < 1 or row["pos"] < 1:
            raise ValueError(f"pileup indels: len is not the length of seq, or unique exceeds reads, in {ln!r}")
        out.append(row)
    return out


def read_indels(path: str) -> list[dict]:
    with open(path) as f:
        return parse_indels(f.read())


def as_read_place(places) -> np.ndarray:
    """mgta_gap_place records -> the mgta_read_place records Context.phase takes: the classic fields, and n_placed = 0 for a read whose
    record is gapped (phase looks at records with n_placed = 1 only, so such a read gives no allele)"""
    places = np.asarray(places, dtype=PLACE_DTYPE)
    out = np.zeros(places.shape, dtype=READ_DTYPE)
    for name in READ_DTYPE.names:
        out[name] = places[name]
    out["n_placed"][places["diag2"] != places["diag"]] = 0
    return out


def main(argv=None) -> int:
    """gapped.py INDELS: checks a PREFIX_pileup_indels.txt and prints its totals"""
    a = list(sys.argv[1:] if argv is None else argv)
    if len(a) != 1:
        print("Usage: python -m megagta_amd.gapped <x_pileup_indels.txt>", file=sys.stderr)
        return 2
    try:
        rows = read_indels(a[0])
    except (ValueError, OSError) as e:
        print("gapped: " + str(e), file=sys.stderr)
        return 1
    for kind in ("ins", "del"):
        sel = [r for r in rows if r["type"] == kind]
        print("%s\t%d events\t%d letters\t%d reads" % (kind, len(sel), sum(r["len"] for r in sel), sum(r["reads"] for r in sel)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
