"""The files of `megagta posterior` / `megagta.py --posterior`: the labels a Viterbi path gives, the PP code, the writers and the
readers, so that tests and users read them one way.  Host only, no device.

  PREFIX_posterior.txt       `#contig<TAB>len<TAB>status<TAB>fwd_nats<TAB>fwd_bits<TAB>viterbi<TAB>mean_pp<TAB>min_pp<TAB>n_below_half`,
                             then one line per input record; status = scored | unaligned; fwd_nats = F, fwd_bits = F / ln 2 and
                             viterbi = the score of mgta_seqs_align's path, each as %.4f (`-inf` when unaligned); mean_pp and min_pp
                             over the residues of that path as %.4f, n_below_half the residues with pp < 0.5 (0.0000, 0.0000 and 0
                             when unaligned); contig = the header up to the first blank
  PREFIX_aligned_pp.fasta    one record per input record, in input order: `>` + the header line as it stood + newline + one line laid
                             out exactly like the record's line in PREFIX_aligned.fasta: per model column the PP code of the residue
                             matched there, or `.` where that row holds `-`; behind a column whose node inserted, the PP code of each
                             inserted residue

The definitions are those of mgta_seqs_posterior (include/megagta_hip.h, INTEGRATION.md 2j′).  The PP code is the one HMMER prints in its
PP lines, restated here and not checked against it."""
from __future__ import annotations

import math

import numpy as np

from .align import record_name  # noqa: F401  (the name of a record is the same in every table)

STATUS = ("scored", "unaligned")
TABLE_HEADER = "#contig\tlen\tstatus\tfwd_nats\tfwd_bits\tviterbi\tmean_pp\tmin_pp\tn_below_half\n"
LN2 = 0.6931471805599453
ROW = np.dtype([("status", np.int32), ("fwd_nats", np.float64), ("fwd_bits", np.float64), ("viterbi", np.float64), ("mean_pp", np.float64),
                ("min_pp", np.float64), ("n_below_half", np.int64)])


def pp_char(p: float) -> str:
    """`*` if p + 0.05 >= 1.0, else the digit floor((p + 0.05) * 10)"""
    q = float(p) + 0.05
    return "*" if q >= 1.0 else "0123456789"[int(math.floor(q * 10.0))]


def labels_from_path(path: str, model_from: int, n_residues: int = 0) -> list:
    """per residue the state that emitted it on a path of mgta_seqs_align over M / I / D that starts in column `model_from`: +j for
    the match state of node j, -j for its insert state.  An empty path is an unaligned record: n_residues times 0 (no state)."""
    if not path:
        return [0] * n_residues
    out, j = [], int(model_from) - 1
    for state in path:
        if state == "M":
            j += 1
            out.append(j)
        elif state == "I":
            out.append(-j)
        elif state == "D":
            j += 1
        else:
            raise ValueError(f"posterior: path state {state!r}")
    return out


def labels_of(align_result: dict, seqs) -> list:
    """the labels of every sequence from the result of Context.align(hmm, seqs, paths=True)"""
    return [labels_from_path(p, int(r["model_from"]), len(s)) for p, r, s in zip(align_result["paths"], align_result["recs"], seqs)]


def pp_line(cols_row, path: str, pp, model_from: int | None = None) -> str:
    """the PP line of one record from its row of `cols` (M bytes), its state path and the posteriors of its residues on that path: as
    long as align.a2m_line of the same record"""
    row = bytes(bytearray(cols_row)).decode("latin-1")
    M = len(row)
    if not path:
        return "." * M
    if model_from is None:
        model_from = next(j + 1 for j, c in enumerate(row) if c != "-")
    out = ["." * (model_from - 1)]
    i, j = 0, model_from - 1
    for state in path:
        if state == "M":
            out.append(pp_char(pp[i]))
            i, j = i + 1, j + 1
        elif state == "D":
            out.append(".")
            j += 1
        elif state == "I":
            out.append(pp_char(pp[i]))
            i += 1
        else:
            raise ValueError(f"posterior: path state {state!r}")
    if i != len(pp) or j > M:
        raise ValueError("posterior: the path does not fit the posteriors and the model")
    out.append("." * (M - j))
    return "".join(out)


def pp_fasta_text(headers, align_result: dict, post_result: dict) -> str:
    """the text of PREFIX_aligned_pp.fasta from Context.align(hmm, seqs, cols=True, paths=True) and Context.posterior(hmm, seqs, labels)"""
    recs, cols, paths, pps = align_result["recs"], align_result["cols"], align_result["paths"], post_result["pp"]
    return "".join(">%s\n%s\n" % (h, pp_line(cols[i], paths[i], pps[i], int(recs["model_from"][i]) or None)) for i, h in enumerate(headers))


def num_text(v: float) -> str:
    return "-inf" if v == float("-inf") else "%.4f" % v


def summary(pp) -> tuple:
    """(mean, minimum, number below 0.5) of the posteriors of one path, added in residue order; (0, 0, 0) for none"""
    n = len(pp)
    if n == 0:
        return 0.0, 0.0, 0
    total, low, below = 0.0, float(pp[0]), 0
    for p in pp:
        p = float(p)
        total += p
        if p < low:
            low = p
        if p < 0.5:
            below += 1
    return total / n, low, below


def table_text(names, lens, align_recs, post_recs, pps) -> str:
    """the text of PREFIX_posterior.txt"""
    rows = [TABLE_HEADER]
    for i, name in enumerate(names):
        r = post_recs[i]
        un = int(r["status"]) != 0
        mean, low, below = (0.0, 0.0, 0) if un else summary(pps[i])
        f = float(r["fwd"])
        rows.append("%s\t%d\t%s\t%s\t%s\t%s\t%.4f\t%.4f\t%d\n" % (name, int(lens[i]), STATUS[1 if un else 0], num_text(f), num_text(f if un else f / LN2),
                                                                 num_text(float("-inf") if un else float(align_recs[i]["score"])), mean, low, below))
    return "".join(rows)


def write_posterior(prefix: str, headers, seqs, align_result: dict, post_result: dict) -> None:
    """PREFIX_posterior.txt and PREFIX_aligned_pp.fasta"""
    with open(prefix + "_posterior.txt", "w") as fh:
        fh.write(table_text([record_name(h) for h in headers], [len(s) for s in seqs], align_result["recs"], post_result["recs"], post_result["pp"]))
    with open(prefix + "_aligned_pp.fasta", "w") as fh:
        fh.write(pp_fasta_text(headers, align_result, post_result))


def parse_table(text: str) -> dict:
    """the text of PREFIX_posterior.txt -> dict(names, lens int64, rows (status 0 scored / 1 unaligned and the numbers as far as %.4f
    kept them))"""
    lines = text.splitlines()
    if not lines or lines[0] + "\n" != TABLE_HEADER:
        raise ValueError("posterior table: the header line is missing")
    names, lens, rows = [], [], []
    for line in lines[1:]:
        f = line.split("\t")
        if len(f) != 9 or f[2] not in STATUS:
            raise ValueError(f"posterior table: bad line {line!r}")
        try:
            row = (STATUS.index(f[2]),) + tuple(float(x) for x in f[3:8]) + (int(f[8]),)
            lens.append(int(f[1]))
        except ValueError:
            raise ValueError(f"posterior table: bad line {line!r}") from None
        if (row[0] == 1) != (row[1] == float("-inf")):
            raise ValueError(f"posterior table: fwd_nats {f[3]} does not go with status {f[2]}")
        names.append(f[0])
        rows.append(row)
    return dict(names=names, lens=np.array(lens, dtype=np.int64), rows=np.array(rows, dtype=ROW))


def read_table(path: str) -> dict:
    with open(path) as fh:
        return parse_table(fh.read())


def parse_pp_fasta(text: str) -> list:
    """the text of PREFIX_aligned_pp.fasta -> [(header, PP line)]"""
    lines = text.splitlines()
    if len(lines) % 2 or not all(h.startswith(">") for h in lines[0::2]):
        raise ValueError("pp fasta: a header line and one PP line per record")
    for s in lines[1::2]:
        if s.strip(".*0123456789"):
            raise ValueError(f"pp fasta: bad PP line {s[:40]!r}")
    return [(h[1:], s) for h, s in zip(lines[0::2], lines[1::2])]


def read_pp_fasta(path: str) -> list:
    with open(path) as fh:
        return parse_pp_fasta(fh.read())
