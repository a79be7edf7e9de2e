"""Per-contig k-mer coverage and abundance files: the two writers `megagta coverage` / `megagta.py --coverage` use and the parser
that reads them back, so that tests and users read the files one way.

  PREFIX_coverage.txt    header `#contig<TAB>len<TAB>windows<TAB>covered<TAB>mean<TAB>median<TAB>min<TAB>max`, then one line per FASTA
                         record in file order; contig = the header up to the first blank; mean = sum / windows as %.4f (0.0000 for a
                         contig shorter than k + 1, which has windows = 0); median = the lower median over all windows, zeros included
  PREFIX_abundance.txt   `multiplicity<TAB>distinct_edges` for every non-empty bin, ascending (no header line)

The format is this project's own (the jar that defined the reference's coverage.txt / abundance.txt is on no machine we have); the
definitions are those of mgta_contig_coverage (include/megagta_hip.h).
"""
from __future__ import annotations

import numpy as np

COVERAGE_HEADER = "#contig\tlen\twindows\tcovered\tmean\tmedian\tmin\tmax"
COLUMNS = ("contig", "len", "windows", "covered", "mean", "median", "min", "max")


def read_fasta(path: str) -> tuple[list[str], list[str]]:
    """-> (names: header up to the first blank, sequences: the record's lines joined), in file order"""
    names, seqs, cur = [], [], None
    with open(path) as fh:
        for line in fh:
            line = line.rstrip("\r\n")
            if line.startswith(">"):
                if cur is not None:
                    seqs.append("".join(cur))
                head = line[1:].split()
                names.append(head[0] if head else "")
                cur = []
            elif cur is not None:
                cur.append(line.strip())
    if cur is not None:
        seqs.append("".join(cur))
    return names, seqs


def stats_of_windows(values, length: int) -> dict:
    """the per-contig row of a list of window coverages (what mgta_contig_coverage computes on the device), in plain numpy"""
    v = np.asarray(values, dtype=np.int64)
    n = int(v.size)
    if n == 0:
        return dict(len=int(length), windows=0, covered=0, sum=0, median=0, min=0, max=0)
    return dict(len=int(length), windows=n, covered=int((v > 0).sum()), sum=int(v.sum()), median=int(np.sort(v)[(n - 1) // 2]),
                min=int(v.min()), max=int(v.max()))


def _row_of_record(c) -> dict:
    """a row of Graph.contig_coverage()['contigs'] (mgta_contig_cov) with the column names of the file"""
    return dict(len=int(c["len"]), windows=int(c["n_windows"]), covered=int(c["n_covered"]), sum=int(c["sum"]), median=int(c["median"]),
                min=int(c["min"]), max=int(c["max"]))


def coverage_text(names, contigs) -> str:
    """names[i] + contigs[i] (a row of Graph.contig_coverage()['contigs'], or a dict as stats_of_windows makes: len / windows / covered / sum /
    median / min / max) -> the text of PREFIX_coverage.txt"""
    out = [COVERAGE_HEADER + "\n"]
    for name, c in zip(names, contigs):
        r = c if isinstance(c, dict) else _row_of_record(c)
        mean = r["sum"] / r["windows"] if r["windows"] else 0.0
        out.append(f"{name}\t{r['len']}\t{r['windows']}\t{r['covered']}\t{mean:.4f}\t{r['median']}\t{r['min']}\t{r['max']}\n")
    return "".join(out)


def abundance_text(abundance) -> str:
    a = np.asarray(abundance, dtype=np.int64)
    return "".join(f"{m}\t{int(a[m])}\n" for m in np.flatnonzero(a))


def write_coverage(path: str, names, contigs) -> None:
    with open(path, "w") as fh:
        fh.write(coverage_text(names, contigs))


def write_abundance(path: str, abundance) -> None:
    with open(path, "w") as fh:
        fh.write(abundance_text(abundance))


def read_coverage(path: str) -> list[dict]:
    """PREFIX_coverage.txt -> one dict per row (contig str, mean float, the rest int), in file order"""
    rows = []
    with open(path) as fh:
        head = fh.readline().rstrip("\n")
        if head != COVERAGE_HEADER:
            raise ValueError(f"{path}: not a coverage file (header {head!r})")
        for line in fh:
            f = line.rstrip("\n").split("\t")
            if len(f) != len(COLUMNS):
                raise ValueError(f"{path}: {len(f)} columns in {line!r}")
            rows.append({c: (v if c == "contig" else float(v) if c == "mean" else int(v)) for c, v in zip(COLUMNS, f)})
    return rows


def read_abundance(path: str) -> np.ndarray:
    """PREFIX_abundance.txt -> int64[65536]"""
    a = np.zeros(65536, dtype=np.int64)
    with open(path) as fh:
        for line in fh:
            m, n = line.split()
            a[int(m)] = int(n)
    return a


def write_for_fasta(graph, fasta_path: str, out_prefix: str) -> dict:
    """the coverage of every record of `fasta_path` on `graph` (loaded with keep_multiplicity) -> out_prefix_coverage.txt and
    out_prefix_abundance.txt; all records go in ONE call, so the abundance counts an edge once for the file.  -> the call's stats"""
    names, seqs = read_fasta(fasta_path)
    res = graph.contig_coverage(seqs)
    write_coverage(out_prefix + "_coverage.txt", names, res["contigs"])
    write_abundance(out_prefix + "_abundance.txt", res["abundance"])
    return res["stats"]
