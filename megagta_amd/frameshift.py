"""The files of `megagta nearest --frameshift` / `megagta.py --frameshift`: the writers and the readers, and what a state path makes of
its nucleotide contig.  Host only, no device.

  PREFIX_frameshift.txt     `#contig<TAB>status<TAB>ref<TAB>score<TAB>identity<TAB>len<TAB>ref_len<TAB>ref_from<TAB>ref_to<TAB>match<TAB>
                            ident<TAB>insert<TAB>delete<TAB>short<TAB>long<TAB>shifts`, then one line per input record in input order.
                            status = aligned | unaligned; ref = the name of the nearest reference; identity = ident / (match + short +
                            long + insert + delete) as %.4f; len = the record's nucleotides, ref_len = the reference's residues;
                            shifts = `.` or a comma list of -i (a short codon that ends at nucleotide i, 1-based) and +i (the dropped
                            letter of a long codon).  An unaligned record has `-` for ref, 0.0000 for identity, `.` for shifts and 0 in
                            every other column but len.
  PREFIX_corr_prot.fasta    the corrected protein of every aligned record, in input order, under its name.
  PREFIX_corr_nucl.fasta    the corrected nucleotides, three per residue of the former.

The definitions are those of mgta_seqs_frameshift (include/megagta_hip.h, INTEGRATION.md 2l').  References and scoring are read as
`nearest` reads them (nearest.read_refs, nearest.parse_scoring).
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .align import record_name

STATUS = ("aligned", "unaligned")
FRAMESHIFT_HEADER = "#contig\tstatus\tref\tscore\tidentity\tlen\tref_len\tref_from\tref_to\tmatch\tident\tinsert\tdelete\tshort\tlong\tshifts\n"
REC = _lib.RECORDS[_lib.FrameshiftRec]                                # mgta_frameshift_rec
CODON_AA = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF"
_NT = {"A": 0, "C": 1, "G": 2, "T": 3, "a": 0, "c": 1, "g": 2, "t": 3}
_TAKES = {"M": 3, "I": 3, "<": 2, ">": 4, "D": 0}


def codon_residue(codon: str) -> str:
    """the residue of three letters by the standard code: X when a letter is not A, C, G, T of either case, `*` for a stop"""
    try:
        return CODON_AA[16 * _NT[codon[0]] + 4 * _NT[codon[1]] + _NT[codon[2]]]
    except KeyError:
        return "X"


def _str(s) -> str:
    return s.decode("latin-1") if isinstance(s, (bytes, bytearray)) else str(s)


def corrected(nucl, path: str) -> tuple:
    """(corrected protein, corrected nucleotides) of a contig under its state path: `M` the residue and its three letters; `>` the
    residue of the last three of four letters, and those three; `<` X and its two letters and N; `I` residue and letters in lower
    case; `D` nothing.  The path must consume exactly the contig."""
    x = _str(nucl)
    prot, nt, pos = [], [], 0
    for s in path:
        take = _TAKES.get(s)
        if take is None or pos + take > len(x):
            raise ValueError(f"frameshift path: {s!r} at nucleotide {pos} of {len(x)}")
        if s == "M" or s == ">":
            pos += s == ">"
            prot.append(codon_residue(x[pos:pos + 3])); nt.append(x[pos:pos + 3])
            pos += 3
        elif s == "<":
            prot.append("X"); nt.append(x[pos:pos + 2] + "N")
            pos += 2
        elif s == "I":
            prot.append(codon_residue(x[pos:pos + 3]).lower()); nt.append(x[pos:pos + 3].lower())
            pos += 3
    if pos != len(x):
        raise ValueError(f"frameshift path: consumes {pos} of {len(x)} nucleotides")
    return "".join(prot), "".join(nt)


def shifts_of(path: str) -> list:
    """the shifts of a path, in path order: -i for a short codon that ends at nucleotide i (1-based), +i for the dropped letter of a
    long codon"""
    out, pos = [], 0
    for s in path:
        if s == "<":
            out.append(-(pos + 2))
        elif s == ">":
            out.append(pos + 1)
        pos += _TAKES[s]
    return out


def shifts_text(shifts) -> str:
    return ",".join("%+d" % v for v in shifts) if len(shifts) else "."


def parse_shifts(text: str) -> list:
    if text == ".":
        return []
    out = [int(f) for f in text.split(",")]
    if any(f[0] not in "+-" for f in text.split(",")) or 0 in out:
        raise ValueError(f"frameshift table: bad shifts {text!r}")
    return out


def identity(rec) -> float:
    """n_ident / (n_match + n_short + n_long + n_insert + n_delete); 0.0 for an unaligned record"""
    cols = int(rec["n_match"]) + int(rec["n_short"]) + int(rec["n_long"]) + int(rec["n_insert"]) + int(rec["n_delete"])
    return int(rec["n_ident"]) / cols if cols else 0.0


def frameshift_text(names, lens, ref_names, ref_lens, recs, paths) -> str:
    """the text of PREFIX_frameshift.txt from the records and paths of Context.frameshift over contigs called `names`, `lens`
    nucleotides long"""
    out = [FRAMESHIFT_HEADER]
    for i, name in enumerate(names):
        r = recs[i]
        un = int(r["status"]) != 0
        out.append("%s\t%s\t%s\t%d\t%.4f\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%s\n" % (
            name, STATUS[int(un)], "-" if un else ref_names[int(r["ref"])], int(r["score"]), identity(r), int(lens[i]), 0 if un else int(ref_lens[int(r["ref"])]),
            int(r["ref_from"]), int(r["ref_to"]), int(r["n_match"]), int(r["n_ident"]), int(r["n_insert"]), int(r["n_delete"]), int(r["n_short"]), int(r["n_long"]),
            "." if un else shifts_text(shifts_of(paths[i]))))
    return "".join(out)


def corrected_texts(names, nucl, recs, paths) -> tuple:
    """(the text of PREFIX_corr_prot.fasta, of PREFIX_corr_nucl.fasta): the aligned records in input order, one line per sequence"""
    prot, nt = [], []
    for i, name in enumerate(names):
        if int(recs[i]["status"]) == 0:
            p, c = corrected(nucl[i], paths[i])
            prot.append(">%s\n%s\n" % (name, p)); nt.append(">%s\n%s\n" % (name, c))
    return "".join(prot), "".join(nt)


def write_frameshift(prefix: str, headers, nucl, ref_names, ref_seqs, result: dict) -> None:
    """PREFIX_frameshift.txt, PREFIX_corr_prot.fasta and PREFIX_corr_nucl.fasta from the result of
    Context.frameshift(nucl, ref_seqs, ..., paths=True)"""
    names = [record_name(h) for h in headers]
    nucl = [_str(s) for s in nucl]
    prot, nt = corrected_texts(names, nucl, result["recs"], result["paths"])
    with open(prefix + "_frameshift.txt", "w", encoding="latin-1") as fh:
        fh.write(frameshift_text(names, [len(s) for s in nucl], ref_names, [len(s) for s in ref_seqs], result["recs"], result["paths"]))
    with open(prefix + "_corr_prot.fasta", "w", encoding="latin-1") as fh:
        fh.write(prot)
    with open(prefix + "_corr_nucl.fasta", "w", encoding="latin-1") as fh:
        fh.write(nt)


def parse_frameshift(text: str) -> dict:
    """the text of PREFIX_frameshift.txt -> dict(names, ref_names (None when unaligned), identity (as far as %.4f kept it), lens,
    ref_lens int64, shifts (a list per record), recs: the fields of mgta_frameshift_rec, ref = -1 throughout: the file names the
    reference, see nearest.ref_index)"""
    lines = text.splitlines()
    if not lines or lines[0] + "\n" != FRAMESHIFT_HEADER:
        raise ValueError("frameshift table: the header line is missing")
    names, ref_names, ident, lens, ref_lens, shifts, rows = [], [], [], [], [], [], []
    for line in lines[1:]:
        f = line.split("\t")
        if len(f) != 16 or f[1] not in STATUS:
            raise ValueError(f"frameshift table: bad line {line!r}")
        try:
            v = [int(x) for x in f[5:15]]
            score, idy, sh = int(f[3]), float(f[4]), parse_shifts(f[15])
        except ValueError:
            raise ValueError(f"frameshift table: bad line {line!r}") from None
        un = f[1] == "unaligned"
        if un != (f[2] == "-") or (un and (score or idy or any(v[1:]) or sh)) or not 0.0 <= idy <= 1.0 or min(v) < 0 or len(sh) != v[8] + v[9]:
            raise ValueError(f"frameshift table: bad line {line!r}")
        names.append(f[0]); ref_names.append(None if un else f[2]); ident.append(idy); lens.append(v[0]); ref_lens.append(v[1]); shifts.append(sh)
        rows.append((int(un), -1, score, v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9]))
    return dict(names=names, ref_names=ref_names, identity=np.array(ident, dtype=np.float64), lens=np.array(lens, dtype=np.int64),
                ref_lens=np.array(ref_lens, dtype=np.int64), shifts=shifts, recs=np.array(rows, dtype=REC))


def read_frameshift(path: str) -> dict:
    with open(path, encoding="latin-1") as fh:
        return parse_frameshift(fh.read())
