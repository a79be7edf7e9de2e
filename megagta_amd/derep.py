"""The files of `megagta derep` / `megagta.py --derep`: the writers and the reader, so that tests and users read them one way.
Host only, no device.

  PREFIX_rmdup.fasta     the kept records in input order: `>` + the header line as it stood + newline + the sequence + newline
  PREFIX_rmdup_map.txt   one line per input record: name <TAB> status <TAB> rep_name <TAB> copies
                         status = kept | duplicate | contained; rep_name = the record's own name (kept), the name of the first record
                         with the same sequence (duplicate), `-` (contained); copies = records equal to a first occurrence, itself
                         included, 0 for a duplicate; name = the header up to the first blank

The definitions are those of mgta_seqs_derep (include/megagta_hip.h).
"""
from __future__ import annotations

import numpy as np

STATUS = ("kept", "duplicate", "contained")


def record_name(header: str) -> str:
    """the name of a record: its header line (without `>`) up to the first blank"""
    return header.split(None, 1)[0] if header.strip() else ""


def map_text(names, status, rep, copies) -> str:
    """the text of PREFIX_rmdup_map.txt from the outputs of Context.derep over records called `names`"""
    rows = []
    for i, name in enumerate(names):
        s = int(status[i])
        rows.append("%s\t%s\t%s\t%d\n" % (name, STATUS[s], "-" if s == 2 else names[int(rep[i])], int(copies[i])))
    return "".join(rows)


def rmdup_fasta_text(headers, seqs, status) -> str:
    """the text of PREFIX_rmdup.fasta: the records whose status is kept, in input order"""
    return "".join(">%s\n%s\n" % (h, s) for h, s, st in zip(headers, seqs, status) if int(st) == 0)


def write_derep(prefix: str, headers, seqs, result: dict) -> None:
    """PREFIX_rmdup.fasta and PREFIX_rmdup_map.txt from the result of Context.derep(seqs)"""
    names = [record_name(h) for h in headers]
    with open(prefix + "_rmdup.fasta", "w") as fh:
        fh.write(rmdup_fasta_text(headers, seqs, result["status"]))
    with open(prefix + "_rmdup_map.txt", "w") as fh:
        fh.write(map_text(names, result["status"], result["rep"], result["copies"]))


def parse_map(text: str) -> dict:
    """the text of a map file -> dict(names, status uint8 (0 kept, 1 duplicate, 2 contained), rep int64 (the index of the record
    rep_name names first; -1 for a contained record), copies uint32)"""
    names, status, rep_names, copies = [], [], [], []
    for line in text.splitlines():
        f = line.split("\t")
        if len(f) != 4 or f[1] not in STATUS or not f[3].isdigit():
            raise ValueError(f"derep map: bad line {line!r}")
        names.append(f[0])
        status.append(STATUS.index(f[1]))
        rep_names.append(f[2])
        copies.append(int(f[3]))
    first = {}
    for i, name in enumerate(names):
        first.setdefault(name, i)
    rep = []
    for i, (s, r) in enumerate(zip(status, rep_names)):
        if (s == 2) != (r == "-") or (s != 2 and r not in first):
            raise ValueError(f"derep map: record {i}: rep_name {r!r} does not go with status {STATUS[s]}")
        rep.append(-1 if s == 2 else first[r])
    return dict(names=names, status=np.array(status, dtype=np.uint8), rep=np.array(rep, dtype=np.int64), copies=np.array(copies, dtype=np.uint32))


def read_map(path: str) -> dict:
    with open(path) as fh:
        return parse_map(fh.read())
