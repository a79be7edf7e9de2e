"""The files of `megagta align` / `megagta.py --align`: the writers and the readers, so that tests and users read them one way.
Host only, no device.

  PREFIX_aligned.fasta   one record per input record, in input order: `>` + the header line as it stood + newline + one line in A2M
                         without dots: for the model's columns 1 .. M in order the column's byte (the upper-cased residue a match
                         state emitted, `-` for a delete state and outside [model_from, model_to]) and, behind a column whose node
                         inserted, the inserted residues in lower case; M times `-` for an unaligned record
  PREFIX_aligned.txt     `#contig<TAB>len<TAB>status<TAB>score<TAB>model_from<TAB>model_to<TAB>match<TAB>insert<TAB>delete`, then one
                         line per input record; status = aligned | unaligned, score as %.4f (`-inf` when unaligned); contig = the
                         header up to the first blank

The definitions are those of mgta_seqs_align (include/megagta_hip.h).
"""
from __future__ import annotations

import numpy as np

from . import _lib

STATUS = ("aligned", "unaligned")
TABLE_HEADER = "#contig\tlen\tstatus\tscore\tmodel_from\tmodel_to\tmatch\tinsert\tdelete\n"
REC = _lib.RECORDS[_lib.AlignRec]                                     # mgta_align_rec


def record_name(header: str) -> str:
    """the name of a record: its header line (without `>`) up to the first blank"""
    return header.split(None, 1)[0] if header.strip() else ""


def _text(s) -> str:
    return s.decode("latin-1") if isinstance(s, (bytes, bytearray)) else str(s)


def a2m_line(cols_row, path: str, seq, model_from: int | None = None) -> str:
    """the A2M line of one record from its row of `cols` (M bytes), its state path and its sequence.  An empty path is an unaligned
    record.  model_from defaults to the first column of the row that is not `-` (a path starts in a match state)."""
    row = bytes(bytearray(cols_row)).decode("latin-1")
    M = len(row)
    if not path:
        return "-" * M
    seq = _text(seq)
    if model_from is None:
        model_from = next(j + 1 for j, c in enumerate(row) if c != "-")
    out = [row[:model_from - 1]]
    i, j = 0, model_from - 1
    for state in path:
        if state == "M":
            out.append(row[j])
            i, j = i + 1, j + 1
        elif state == "D":
            out.append(row[j])
            j += 1
        elif state == "I":
            out.append(seq[i].lower() if "A" <= seq[i] <= "Z" else seq[i])
            i += 1
        else:
            raise ValueError(f"align path: state {state!r}")
    if i != len(seq) or j > M:
        raise ValueError("align path: does not fit the sequence and the model")
    out.append(row[j:])
    return "".join(out)


def aligned_fasta_text(headers, seqs, result: dict) -> str:
    """the text of PREFIX_aligned.fasta from the result of Context.align(hmm, seqs, cols=True, paths=True)"""
    recs, cols, paths = result["recs"], result["cols"], result["paths"]
    return "".join(">%s\n%s\n" % (h, a2m_line(cols[i], paths[i], s, int(recs["model_from"][i]) or None)) for i, (h, s) in enumerate(zip(headers, seqs)))


def score_text(score: float) -> str:
    return "-inf" if score == float("-inf") else "%.4f" % score


def table_text(names, lens, recs) -> str:
    """the text of PREFIX_aligned.txt from the records of Context.align over sequences called `names`, `lens` residues long"""
    rows = [TABLE_HEADER]
    for i, name in enumerate(names):
        r = recs[i]
        rows.append("%s\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\n" % (name, int(lens[i]), STATUS[int(r["status"])], score_text(float(r["score"])), int(r["model_from"]),
                                                              int(r["model_to"]), int(r["n_match"]), int(r["n_insert"]), int(r["n_delete"])))
    return "".join(rows)


def write_align(prefix: str, headers, seqs, result: dict) -> None:
    """PREFIX_aligned.fasta and PREFIX_aligned.txt from the result of Context.align(hmm, seqs, cols=True, paths=True)"""
    with open(prefix + "_aligned.fasta", "w") as fh:
        fh.write(aligned_fasta_text(headers, seqs, result))
    with open(prefix + "_aligned.txt", "w") as fh:
        fh.write(table_text([record_name(h) for h in headers], [len(s) for s in seqs], result["recs"]))


def parse_table(text: str) -> dict:
    """the text of PREFIX_aligned.txt -> dict(names, lens int64, recs (the fields of mgta_align_rec; score as far as %.4f kept it))"""
    lines = text.splitlines()
    if not lines or lines[0] + "\n" != TABLE_HEADER:
        raise ValueError("align table: the header line is missing")
    names, lens, rows = [], [], []
    for line in lines[1:]:
        f = line.split("\t")
        if len(f) != 9 or f[2] not in STATUS:
            raise ValueError(f"align table: bad line {line!r}")
        try:
            row = (float(f[3]), STATUS.index(f[2])) + tuple(int(x) for x in f[4:])
            lens.append(int(f[1]))
        except ValueError:
            raise ValueError(f"align table: bad line {line!r}") from None
        if (row[1] == 1) != (row[0] == float("-inf")):
            raise ValueError(f"align table: score {f[3]} does not go with status {f[2]}")
        names.append(f[0])
        rows.append(row)
    return dict(names=names, lens=np.array(lens, dtype=np.int64), recs=np.array(rows, dtype=REC))


def read_table(path: str) -> dict:
    with open(path) as fh:
        return parse_table(fh.read())


def parse_aligned_fasta(text: str) -> list:
    """the text of PREFIX_aligned.fasta -> [(header, A2M line)]"""
    lines = text.splitlines()
    if len(lines) % 2 or not all(h.startswith(">") for h in lines[0::2]):
        raise ValueError("aligned fasta: a header line and one sequence line per record")
    return [(h[1:], s) for h, s in zip(lines[0::2], lines[1::2])]


def read_aligned_fasta(path: str) -> list:
    with open(path) as fh:
        return parse_aligned_fasta(fh.read())


def a2m_columns(line: str) -> str:
    """the model's columns of an A2M line: the line without its lower-case (inserted) residues -- the row of `cols`"""
    return "".join(c for c in line if not "a" <= c <= "z")
