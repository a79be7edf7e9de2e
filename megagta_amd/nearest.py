"""The files of `megagta nearest` / `megagta.py --nearest`: the writers and the readers, so that tests and users read them one way.
Host only, no device.

  PREFIX_nearest.txt        `#contig<TAB>status<TAB>ref<TAB>score<TAB>identity<TAB>len<TAB>ref_len<TAB>ref_from<TAB>ref_to<TAB>match<TAB>
                            ident<TAB>insert<TAB>delete`, then one line per input record in input order.  status = aligned | unaligned;
                            ref = the name of the nearest reference; identity = ident / (match + insert + delete) as %.4f; len = the
                            record's residues, ref_len = the reference's.  An unaligned record (no reference gives it a score) has `-`
                            for ref, 0.0000 for identity and 0 in every other column but len.
  PREFIX_nearest_refs.txt   `#ref<TAB>ref_len<TAB>contigs<TAB>mean_identity`, then one line per reference in file order: the records it
                            is nearest to and the mean of their identities as %.4f; 0 and 0.0000 for a reference nearest to none.

The references: name = the header up to the first blank, residues = the record's ASCII letters, upper-cased; `-`, `.`, `*` and
everything else are dropped, so the file may be an alignment.  Scoring is `MATCH,MISMATCH` (two integers) or the path of a matrix file
in NCBI format.  The definitions are those of mgta_seqs_nearest (include/megagta_hip.h).
"""
from __future__ import annotations

import os

import numpy as np

from . import _lib
from .align import record_name

STATUS = ("aligned", "unaligned")
NEAREST_HEADER = "#contig\tstatus\tref\tscore\tidentity\tlen\tref_len\tref_from\tref_to\tmatch\tident\tinsert\tdelete\n"
REFS_HEADER = "#ref\tref_len\tcontigs\tmean_identity\n"
REC = _lib.RECORDS[_lib.NearestRec]                                   # mgta_nearest_rec
_LETTERS = "ABCDEFGHIJKLMNOPQRSTUVWXYZ"


def residue_class(b: int) -> int:
    """c(b): 1 .. 26 for an ASCII letter of either case, 0 for every other byte"""
    return (b | 32) - 96 if b < 128 and 97 <= (b | 32) <= 122 else 0


def parse_fasta(text: str) -> list:
    """[(header line without `>`, the record's lines joined)]; lines before the first header are dropped"""
    out, cur = [], None
    for line in text.splitlines():
        if line.startswith(">"):
            cur = [line[1:], []]
            out.append(cur)
        elif cur is not None:
            cur[1].append(line.strip(" \t"))
    return [(h, "".join(parts)) for h, parts in out]


def parse_refs(text: str) -> tuple:
    """the reference set of a FASTA text, aligned or not -> (names, sequences): ASCII letters only, upper-cased"""
    names, seqs = [], []
    for h, s in parse_fasta(text):
        names.append(record_name(h))
        seqs.append("".join(c.upper() for c in s if c.isascii() and c.isalpha()))
    return names, seqs


def read_refs(path: str) -> tuple:
    with open(path, encoding="latin-1") as fh:
        return parse_refs(fh.read())


def match_mismatch(match: int, mismatch: int) -> np.ndarray:
    """sub[a][b] = match when a == b != 0, else mismatch"""
    for v in (match, mismatch):
        if not -128 <= v <= 127:
            raise ValueError(f"nearest scoring: {v} is outside int8")
    sub = np.full((27, 27), mismatch, dtype=np.int8)
    for a in range(1, 27):
        sub[a, a] = match
    return sub


def parse_matrix(text: str) -> np.ndarray:
    """a substitution matrix in NCBI format -> int8[27, 27]: `#` comments, a header row of letters, rows `LETTER v v ...`; a `*` row or
    column fills class 0; letters the file does not have take its lowest value; a value outside int8 and a ragged row are errors"""
    cols, rows = None, {}
    for line in text.splitlines():
        line = line.split("#", 1)[0].strip()
        if not line:
            continue
        f = line.split()
        if cols is None:
            cols = f
            if len(set(cols)) != len(cols) or not all(len(c) == 1 and (c == "*" or (c.isascii() and c.isalpha())) for c in cols):
                raise ValueError(f"nearest matrix: bad header row {line!r}")
            continue
        if len(f) != len(cols) + 1 or f[0] not in cols or f[0] in rows:
            raise ValueError(f"nearest matrix: bad row {line!r}")
        try:
            vals = [int(v) for v in f[1:]]
        except ValueError:
            raise ValueError(f"nearest matrix: bad row {line!r}") from None
        if any(not -128 <= v <= 127 for v in vals):
            raise ValueError(f"nearest matrix: a value of row {f[0]} is outside int8")
        rows[f[0]] = vals
    if cols is None or set(rows) != set(cols):
        raise ValueError("nearest matrix: a header row of letters and one row per letter of it")
    cls = {c: (0 if c == "*" else residue_class(ord(c))) for c in cols}
    if len(set(cls.values())) != len(cls):
        raise ValueError("nearest matrix: a letter is there in both cases")
    sub = np.full((27, 27), min(min(v) for v in rows.values()), dtype=np.int8)
    for a in cols:
        for b, v in zip(cols, rows[a]):
            sub[cls[a], cls[b]] = v
    return sub


def parse_scoring(spec: str) -> np.ndarray:
    """`MATCH,MISMATCH` or the path of a matrix file -> int8[27, 27]"""
    parts = spec.split(",")
    if len(parts) == 2:
        try:
            return match_mismatch(int(parts[0]), int(parts[1]))
        except ValueError as e:
            if not os.path.exists(spec):
                raise ValueError(f"nearest scoring: {spec!r} is neither MATCH,MISMATCH nor a matrix file ({e})") from None
    with open(spec, encoding="latin-1") as fh:
        return parse_matrix(fh.read())


def identity(rec) -> float:
    """n_ident / (n_match + n_insert + n_delete); 0.0 for an unaligned record"""
    cols = int(rec["n_match"]) + int(rec["n_insert"]) + int(rec["n_delete"])
    return int(rec["n_ident"]) / cols if cols else 0.0


def nearest_text(names, lens, ref_names, ref_lens, recs) -> str:
    """the text of PREFIX_nearest.txt from the records of Context.nearest over contigs called `names`, `lens` residues long"""
    out = [NEAREST_HEADER]
    for i, name in enumerate(names):
        r = recs[i]
        un = int(r["status"]) != 0
        out.append("%s\t%s\t%s\t%d\t%.4f\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (
            name, STATUS[int(un)], "-" if un else ref_names[int(r["ref"])], int(r["score"]), identity(r), int(lens[i]), 0 if un else int(ref_lens[int(r["ref"])]),
            int(r["ref_from"]), int(r["ref_to"]), int(r["n_match"]), int(r["n_ident"]), int(r["n_insert"]), int(r["n_delete"])))
    return "".join(out)


def refs_text(ref_names, ref_lens, recs) -> str:
    """the text of PREFIX_nearest_refs.txt: per reference the contigs it is nearest to and the mean of their identities (summed in
    input order, divided once)"""
    count, total = [0] * len(ref_names), [0.0] * len(ref_names)
    for r in recs:
        if int(r["status"]) == 0:
            count[int(r["ref"])] += 1
            total[int(r["ref"])] += identity(r)
    return REFS_HEADER + "".join("%s\t%d\t%d\t%.4f\n" % (name, int(ref_lens[j]), count[j], total[j] / count[j] if count[j] else 0.0)
                                 for j, name in enumerate(ref_names))


def write_nearest(prefix: str, headers, seqs, ref_names, ref_seqs, result: dict) -> None:
    """PREFIX_nearest.txt and PREFIX_nearest_refs.txt from the result of Context.nearest(seqs, ref_seqs, ...)"""
    ref_lens = [len(s) for s in ref_seqs]
    with open(prefix + "_nearest.txt", "w", encoding="latin-1") as fh:
        fh.write(nearest_text([record_name(h) for h in headers], [len(s) for s in seqs], ref_names, ref_lens, result["recs"]))
    with open(prefix + "_nearest_refs.txt", "w", encoding="latin-1") as fh:
        fh.write(refs_text(ref_names, ref_lens, result["recs"]))


def parse_nearest(text: str) -> dict:
    """the text of PREFIX_nearest.txt -> dict(names, ref_names (None when unaligned), identity (as far as %.4f kept it), lens, ref_lens
    int64, recs: the fields of mgta_nearest_rec, ref = -1 throughout: the file names the reference, see ref_index)"""
    lines = text.splitlines()
    if not lines or lines[0] + "\n" != NEAREST_HEADER:
        raise ValueError("nearest table: the header line is missing")
    names, ref_names, ident, lens, ref_lens, rows = [], [], [], [], [], []
    for line in lines[1:]:
        f = line.split("\t")
        if len(f) != 13 or f[1] not in STATUS:
            raise ValueError(f"nearest table: bad line {line!r}")
        try:
            v = [int(x) for x in f[5:]]
            score, idy = int(f[3]), float(f[4])
        except ValueError:
            raise ValueError(f"nearest table: bad line {line!r}") from None
        un = f[1] == "unaligned"
        if un != (f[2] == "-") or (un and (score or idy or any(v[1:]))) or not 0.0 <= idy <= 1.0 or min(v) < 0:
            raise ValueError(f"nearest table: bad line {line!r}")
        names.append(f[0]); ref_names.append(None if un else f[2]); ident.append(idy); lens.append(v[0]); ref_lens.append(v[1])
        rows.append((int(un), -1, score, v[2], v[3], v[4], v[5], v[6], v[7]))
    return dict(names=names, ref_names=ref_names, identity=np.array(ident, dtype=np.float64), lens=np.array(lens, dtype=np.int64),
                ref_lens=np.array(ref_lens, dtype=np.int64), recs=np.array(rows, dtype=REC))


def read_nearest(path: str) -> dict:
    with open(path, encoding="latin-1") as fh:
        return parse_nearest(fh.read())


def parse_refs_table(text: str) -> dict:
    """the text of PREFIX_nearest_refs.txt -> dict(names, ref_lens int64, contigs int64, mean_identity float64)"""
    lines = text.splitlines()
    if not lines or lines[0] + "\n" != REFS_HEADER:
        raise ValueError("nearest refs table: the header line is missing")
    names, rl, cnt, mean = [], [], [], []
    for line in lines[1:]:
        f = line.split("\t")
        try:
            if len(f) != 4:
                raise ValueError
            row = (int(f[1]), int(f[2]), float(f[3]))
        except ValueError:
            raise ValueError(f"nearest refs table: bad line {line!r}") from None
        if min(row) < 0 or row[2] > 1.0 or (row[1] == 0 and row[2] != 0.0):
            raise ValueError(f"nearest refs table: bad line {line!r}")
        names.append(f[0]); rl.append(row[0]); cnt.append(row[1]); mean.append(row[2])
    return dict(names=names, ref_lens=np.array(rl, dtype=np.int64), contigs=np.array(cnt, dtype=np.int64), mean_identity=np.array(mean, dtype=np.float64))


def read_refs_table(path: str) -> dict:
    with open(path, encoding="latin-1") as fh:
        return parse_refs_table(fh.read())


def ref_index(ref_names) -> dict:
    """name -> the first reference of that name, to turn the `ref` column of PREFIX_nearest.txt back into an index"""
    first = {}
    for j, name in enumerate(ref_names):
        first.setdefault(name, j)
    return first
