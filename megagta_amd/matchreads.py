"""The matched-reads file of `megagta matchreads` / `megagta.py --match-reads`: the writer and the reader, so that tests and users
read the file one way.  Host only, no device.

  PREFIX_match_reads.fa   one record `>r<i>` + newline + the read as sequenced + newline per matched read, ascending i; i = the
                          0-based index of the read in the library (the library keeps no names; an N of the input is a G there)

The definitions are those of mgta_reads_match_contigs (include/megagta_hip.h).
"""
from __future__ import annotations

import numpy as np

_DNA = np.frombuffer(b"ACGT", dtype=np.uint8)


def read_codes(packed: np.ndarray, start: np.ndarray, i: int, reversed_storage: bool = True) -> np.ndarray:
    """base codes (A0 C1 G2 T3) of read i as sequenced, from the packed library as it is uploaded: 2 bits per base, base j of a word
    at bits 30 - 2j, reads back to back from start[i] (in bases), every read stored reversed when reversed_storage"""
    q = np.arange(int(start[i]), int(start[i + 1]), dtype=np.int64)
    codes = ((packed[q >> 4] >> (30 - 2 * (q & 15)).astype(np.uint32)) & 3).astype(np.uint8)
    return codes[::-1] if reversed_storage else codes


def match_reads_text(indices, packed: np.ndarray, start: np.ndarray, reversed_storage: bool = True) -> str:
    """the text of PREFIX_match_reads.fa for the reads `indices` (any order, given once each; or a bool mask over the reads)"""
    idx = np.asarray(indices)
    idx = np.flatnonzero(idx) if idx.dtype == bool else np.sort(idx.astype(np.int64))
    packed = np.asarray(packed, dtype=np.uint32)
    return "".join(">r%d\n%s\n" % (i, _DNA[read_codes(packed, start, int(i), reversed_storage)].tobytes().decode()) for i in idx)


def write_match_reads(path: str, indices, packed: np.ndarray, start: np.ndarray, reversed_storage: bool = True) -> None:
    with open(path, "w") as fh:
        fh.write(match_reads_text(indices, packed, start, reversed_storage))


def parse_match_reads(text: str) -> tuple[np.ndarray, list[str]]:
    """the text of a matched-reads file -> (read indices int64, sequences)"""
    lines = text.splitlines()
    if len(lines) % 2:
        raise ValueError("matched-reads text: a record is a header line and a sequence line")
    idx, seqs = [], []
    for head, seq in zip(lines[0::2], lines[1::2]):
        if not head.startswith(">r") or not head[2:].isdigit():
            raise ValueError(f"matched-reads text: bad header {head!r}")
        idx.append(int(head[2:]))
        seqs.append(seq)
    return np.array(idx, dtype=np.int64), seqs


def read_match_reads(path: str) -> tuple[np.ndarray, list[str]]:
    with open(path) as fh:
        return parse_match_reads(fh.read())
