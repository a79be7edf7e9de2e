"""The files of `megagta chimera` / `megagta.py --chimera`: the writers and the readers, so that tests and users read them one way.
Host only, no device.

  PREFIX_chimera.txt     `#contig<TAB>status<TAB>ref<TAB>score<TAB>len<TAB>break<TAB>left_ref<TAB>left_score<TAB>right_ref<TAB>right_score<TAB>
                         two<TAB>one<TAB>gain`, then one line per input record in input order.  status = clean | chimeric | unchecked;
                         ref = the name of the nearest reference and score its score; break = the residues left of the break; left_ref
                         and right_ref = the two parents.  An absent reference is `-`; an unchecked record has 0 from `break` on and
                         `-` for both parents.
  PREFIX_nochim.fasta    the records that are not chimeric, as they were read.

References and scoring are read by megagta_amd.nearest.  The definitions are those of mgta_seqs_chimera (include/megagta_hip.h,
INTEGRATION.md 2m); the rule is this project's own, not uchime's.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .align import record_name

STATUS = ("clean", "chimeric", "unchecked")
CHIMERA_HEADER = "#contig\tstatus\tref\tscore\tlen\tbreak\tleft_ref\tleft_score\tright_ref\tright_score\ttwo\tone\tgain\n"
REC = _lib.RECORDS[_lib.ChimeraRec]                                   # mgta_chimera_rec
UNCHECKED = (2, -1, 0, 0, -1, 0, -1, 0, 0, 0, 0)
MIN_SEG_RANGE, MIN_GAIN_RANGE = (1, 4096), (1, 1 << 20)


def chimera_text(names, lens, ref_names, recs) -> str:
    """the text of PREFIX_chimera.txt from the records of Context.chimera over contigs called `names`, `lens` residues long"""
    def ref(j):
        return "-" if int(j) < 0 else ref_names[int(j)]

    out = [CHIMERA_HEADER]
    for i, name in enumerate(names):
        r = recs[i]
        out.append("%s\t%s\t%s\t%d\t%d\t%d\t%s\t%d\t%s\t%d\t%d\t%d\t%d\n" % (
            name, STATUS[int(r["status"])], ref(r["ref"]), int(r["score"]), int(lens[i]), int(r["brk"]), ref(r["left_ref"]), int(r["left_score"]),
            ref(r["right_ref"]), int(r["right_score"]), int(r["two"]), int(r["one"]), int(r["gain"])))
    return "".join(out)


def nochim_text(headers, seqs, recs) -> str:
    """the text of PREFIX_nochim.fasta: the records that are not chimeric"""
    return "".join(">%s\n%s\n" % (h, s) for h, s, r in zip(headers, seqs, recs) if int(r["status"]) != 1)


def write_chimera(prefix: str, headers, seqs, ref_names, result: dict) -> None:
    """PREFIX_chimera.txt and PREFIX_nochim.fasta from the result of Context.chimera(seqs, ref_seqs, ...)"""
    with open(prefix + "_chimera.txt", "w", encoding="latin-1") as fh:
        fh.write(chimera_text([record_name(h) for h in headers], [len(s) for s in seqs], ref_names, result["recs"]))
    with open(prefix + "_nochim.fasta", "w", encoding="latin-1") as fh:
        fh.write(nochim_text(headers, seqs, result["recs"]))


def parse_chimera(text: str) -> dict:
    """the text of PREFIX_chimera.txt -> dict(names, ref_names, left_names, right_names (None where absent), lens int64, recs: the
    fields of mgta_chimera_rec with ref = left_ref = right_ref = -1 throughout: the file names the references, see
    megagta_amd.nearest.ref_index)"""
    lines = text.splitlines()
    if not lines or lines[0] + "\n" != CHIMERA_HEADER:
        raise ValueError("chimera table: the header line is missing")
    names, refs, lefts, rights, lens, rows = [], [], [], [], [], []
    for line in lines[1:]:
        f = line.split("\t")
        if len(f) != 13 or f[1] not in STATUS or not f[2] or not f[6] or not f[8]:
            raise ValueError(f"chimera table: bad line {line!r}")
        try:
            score, length, brk, ls, rs, two, one, gain = (int(f[k]) for k in (3, 4, 5, 7, 9, 10, 11, 12))
        except ValueError:
            raise ValueError(f"chimera table: bad line {line!r}") from None
        status = STATUS.index(f[1])
        bad = length < 0 or brk < 0 or brk > length or (f[2] == "-" and score != 0) or gain != two - one or two != ls + rs
        if status == 2:
            bad = bad or f[6] != "-" or f[8] != "-" or any((brk, ls, rs, two, one, gain))
        else:
            bad = bad or f[6] == "-" or f[8] == "-" or not 1 <= brk < length
        if bad:
            raise ValueError(f"chimera table: bad line {line!r}")
        names.append(f[0]); lens.append(length)
        refs.append(None if f[2] == "-" else f[2]); lefts.append(None if f[6] == "-" else f[6]); rights.append(None if f[8] == "-" else f[8])
        rows.append((status, -1, score, brk, -1, ls, -1, rs, two, one, gain))
    return dict(names=names, ref_names=refs, left_names=lefts, right_names=rights, lens=np.array(lens, dtype=np.int64), recs=np.array(rows, dtype=REC))


def read_chimera(path: str) -> dict:
    with open(path, encoding="latin-1") as fh:
        return parse_chimera(fh.read())
