"""The files of `megagta samplecov` and of `megagta.py --sample-abund`: the writers, the readers and the join that turns the per-library
coverage of a gene's contigs into a cluster x sample table.  Host only, no device; masses and ppm in integers only.

  PREFIX_samplecov.txt         one line `#lib<TAB>s<TAB>reads<TAB>read_windows<TAB>hit_windows<TAB>text` per library (s counts from 1, text is
                               the library's line of `.lib_info`), then `#contig<TAB>len<TAB>windows<TAB>covered<TAB>unique<TAB>max_share<TAB>
                               mass_1 ... mass_L`, then one line per FASTA record in file order (mgta_contig_sample_coverage over the whole
                               file in one call).  A mass is the record's Q16 mass in that library printed with four decimals by the
                               integer rule of megagta_amd/taxonabund.py, so the C++ host and this module print the same bytes.
  PREFIX_otu_samples.txt       the `#lib` lines, then `#cluster<TAB>rep<TAB>contigs<TAB>mass_1 ... mass_L`, one line per cluster of
                               PREFIX_clust.txt in cluster order, a line `-<TAB>-<TAB>n<TAB>...` for the n > 0 unaligned records, and a
                               closing line `#total<TAB>-<TAB>records<TAB>...`.
  PREFIX_otu_samples_ppm.txt   the same rows with floor(mass * 10^6 / total_s) in place of every mass, 0 where a library's total is 0.

From the file on a mass is an integer number of ten-thousandths: the tables are summed in that unit, so every column of
PREFIX_otu_samples.txt sums to its `#total` exactly.  The ppm are floors and sum to at most 10^6 per library.  The definitions are this
project's own.
"""
from __future__ import annotations

import sys

import numpy as np

from .taxonabund import _MASS, e4_text, parse_e4, ppm_of, q16_text

LIB_TAG = "#lib"
CONTIG_COLUMNS = ("#contig", "len", "windows", "covered", "unique", "max_share")
OTU_COLUMNS = ("#cluster", "rep", "contigs")
TOTAL_TAG = "#total"


def _header(columns, n_libs: int) -> str:
    return "\t".join(columns + tuple("mass_%d" % (s + 1) for s in range(n_libs))) + "\n"


def lib_read_windows(start, lib_end, k: int) -> list:
    """sum max(0, len - k) over the reads of every library: start = the [n + 1] base offsets of an upload, lib_end as for
    Graph.contig_sample_coverage"""
    lens = np.diff(np.asarray(start, dtype=np.uint64).astype(np.int64))
    below = np.zeros(lens.size + 1, dtype=np.int64)
    np.cumsum(np.maximum(0, lens - int(k)), out=below[1:])
    ends = [0] + [int(e) for e in lib_end]
    return [int(below[b] - below[a]) for a, b in zip(ends, ends[1:])]


def libs_of(lib_table, read_windows, hit_windows) -> list:
    """readlib.read_lib_table rows + the two window counts per library -> the library records of the writers"""
    return [dict(reads=to - frm + 1, read_windows=int(rw), hit_windows=int(hw), text=text)
            for (text, frm, to, _, _), rw, hw in zip(lib_table, read_windows, hit_windows)]


def lib_lines(libs) -> str:
    return "".join("%s\t%d\t%d\t%d\t%d\t%s\n" % (LIB_TAG, s + 1, lib["reads"], lib["read_windows"], lib["hit_windows"], lib["text"]) for s, lib in enumerate(libs))


# ---- PREFIX_samplecov.txt -------------------------------------------------------------------------------------------------------------
def samplecov_text(libs, names, contigs, mass) -> str:
    """libs: dict(reads, read_windows, hit_windows, text) per library; names[i] + contigs[i] (a row of
    Graph.contig_sample_coverage()['contigs']) + mass[i] (its Q16 masses, one per library) -> the text of PREFIX_samplecov.txt"""
    out = [lib_lines(libs), _header(CONTIG_COLUMNS, len(libs))]
    for name, c, m in zip(names, contigs, mass):
        if len(m) != len(libs):
            raise ValueError(f"samplecov: {len(m)} masses for {len(libs)} libraries")
        out.append("%s\t%d\t%d\t%d\t%d\t%d" % (name, int(c["len"]), int(c["n_windows"]), int(c["n_covered"]), int(c["n_unique"]), int(c["max_share"])))
        out.append("".join("\t" + q16_text(int(x)) for x in m) + "\n")
    return "".join(out)


def _parse_libs(lines, what: str):
    libs = []
    while len(libs) < len(lines) and lines[len(libs)].startswith(LIB_TAG + "\t"):
        f = lines[len(libs)].split("\t", 5)
        if len(f) != 6 or not all(x.isdigit() for x in f[1:5]) or int(f[1]) != len(libs) + 1 or int(f[4]) > int(f[3]):
            raise ValueError(f"{what}: bad line {lines[len(libs)]!r}")
        libs.append(dict(reads=int(f[2]), read_windows=int(f[3]), hit_windows=int(f[4]), text=f[5]))
    if not libs:
        raise ValueError(f"{what}: no #lib line")
    return libs


def parse_samplecov(text: str) -> dict:
    """the text of PREFIX_samplecov.txt -> dict(libs = the library records, rows = one dict per record in file order: contig str, len /
    windows / covered / unique / max_share int, mass = list of int in ten-thousandths, one per library)"""
    lines = text.splitlines()
    libs = _parse_libs(lines, "samplecov table")
    n_libs = len(libs)
    if len(lines) <= n_libs or lines[n_libs] + "\n" != _header(CONTIG_COLUMNS, n_libs):
        raise ValueError("samplecov table: the header line is missing")
    rows = []
    for line in lines[n_libs + 1:]:
        f = line.split("\t")
        if len(f) != 6 + n_libs or not all(x.isdigit() for x in f[1:6]) or not all(_MASS.match(x) for x in f[6:]):
            raise ValueError(f"samplecov table: bad line {line!r}")
        r = dict(contig=f[0], len=int(f[1]), windows=int(f[2]), covered=int(f[3]), unique=int(f[4]), max_share=int(f[5]), mass=[parse_e4(x) for x in f[6:]])
        if r["covered"] > r["windows"] or r["unique"] > r["covered"] or (r["covered"] == 0) != (r["max_share"] == 0) or (r["covered"] == 0 and any(r["mass"])):
            raise ValueError(f"samplecov table: bad line {line!r}")
        rows.append(r)
    return dict(libs=libs, rows=rows)


def read_samplecov(path: str) -> dict:
    with open(path, encoding="latin-1") as fh:
        return parse_samplecov(fh.read())


# ---- the join -------------------------------------------------------------------------------------------------------------------------
def join(samplecov: dict, clust: dict) -> dict:
    """samplecov: parse_samplecov over the nucleotide records; clust: megagta_amd.cluster.parse_clust of the protein records, one per
    nucleotide record, position by position and under the same name.  -> dict(libs, rows = one dict(cluster, rep, contigs, mass) per
    cluster in cluster order and a last one with cluster = rep = None for the unaligned records when there are any, records, total =
    the column sums), masses in ten-thousandths.  Any mismatch is a ValueError: nothing is guessed."""
    rows_in, names = samplecov["rows"], list(clust["names"])
    n_libs = len(samplecov["libs"])
    if len(rows_in) != len(names):
        raise ValueError(f"samplecov: {len(rows_in)} nucleotide records, {len(names)} lines in the cluster table")
    for i, (r, name) in enumerate(zip(rows_in, names)):
        if r["contig"] != name:
            raise ValueError(f"samplecov: record {i} is {r['contig']!r} in the nucleotide file and {name!r} in the cluster table")
    clusters, un_n, un_mass = {}, 0, [0] * n_libs
    for i, r in enumerate(rows_in):
        if int(clust["status"][i]) == 2:
            un_n += 1
            un_mass = [a + b for a, b in zip(un_mass, r["mass"])]
            continue
        rep = names[int(clust["rep"][i])]
        c = clusters.setdefault(int(clust["cluster"][i]), dict(rep=rep, contigs=0, mass=[0] * n_libs))
        if c["rep"] != rep:
            raise ValueError(f"samplecov: cluster {int(clust['cluster'][i])} has two representatives")
        c["contigs"] += 1
        c["mass"] = [a + b for a, b in zip(c["mass"], r["mass"])]
    rows = [dict(cluster=number, rep=clusters[number]["rep"], contigs=clusters[number]["contigs"], mass=clusters[number]["mass"]) for number in sorted(clusters)]
    if un_n:
        rows.append(dict(cluster=None, rep=None, contigs=un_n, mass=un_mass))
    total = [sum(r["mass"][s] for r in rows_in) for s in range(n_libs)]
    return dict(libs=samplecov["libs"], rows=rows, records=len(rows_in), total=total)


# ---- PREFIX_otu_samples.txt and PREFIX_otu_samples_ppm.txt ----------------------------------------------------------------------------
def _otu_lines(table: dict, cell) -> str:
    n_libs = len(table["libs"])
    out = [lib_lines(table["libs"]), _header(OTU_COLUMNS, n_libs)]
    for r in table["rows"]:
        out.append("%s\t%s\t%d" % ("-" if r["cluster"] is None else r["cluster"], r["rep"] or "-", r["contigs"]))
        out.append("".join("\t" + cell(r["mass"][s], s) for s in range(n_libs)) + "\n")
    out.append("%s\t-\t%d" % (TOTAL_TAG, table["records"]))
    out.append("".join("\t" + cell(table["total"][s], s) for s in range(n_libs)) + "\n")
    return "".join(out)


def otu_samples_text(table: dict) -> str:
    """the result of join -> the text of PREFIX_otu_samples.txt"""
    return _otu_lines(table, lambda m, s: e4_text(m))


def otu_samples_ppm_text(table: dict) -> str:
    """the result of join -> the text of PREFIX_otu_samples_ppm.txt (the closing line holds the ppm of the totals: 10^6, or 0)"""
    return _otu_lines(table, lambda m, s: "%d" % ppm_of(m, table["total"][s]))


def _parse_otu(text: str, what: str, cell_ok, cell) -> dict:
    lines = text.splitlines()
    libs = _parse_libs(lines, what)
    n_libs = len(libs)
    if len(lines) <= n_libs + 1 or lines[n_libs] + "\n" != _header(OTU_COLUMNS, n_libs):
        raise ValueError(f"{what}: the header line is missing")
    rows = []
    body = lines[n_libs + 1:]
    for n, line in enumerate(body):
        f = line.split("\t")
        ok = len(f) == 3 + n_libs and f[2].isdigit() and all(cell_ok(x) for x in f[3:])
        if ok and n == len(body) - 1:                                     # the closing line
            ok = f[0] == TOTAL_TAG and f[1] == "-"
        elif ok and f[0] == "-":                                          # the unaligned records: the line before the closing one
            ok = f[1] == "-" and int(f[2]) > 0 and n == len(body) - 2
        elif ok:
            ok = f[0].isdigit() and f[1] not in ("", "-") and int(f[2]) > 0
        if not ok:
            raise ValueError(f"{what}: bad line {line!r}")
        rows.append(dict(cluster=int(f[0]) if f[0].isdigit() else None, rep=None if f[1] == "-" else f[1], contigs=int(f[2]), mass=[cell(x) for x in f[3:]]))
    last = rows.pop()
    if sum(r["contigs"] for r in rows) != last["contigs"]:
        raise ValueError(f"{what}: the lines hold {sum(r['contigs'] for r in rows)} records, the closing line says {last['contigs']}")
    return dict(libs=libs, rows=rows, records=last["contigs"], total=last["mass"])


def parse_otu_samples(text: str) -> dict:
    """the text of PREFIX_otu_samples.txt -> what join returned; a column that does not sum to its total is an error"""
    table = _parse_otu(text, "otu samples table", lambda x: bool(_MASS.match(x)), parse_e4)
    for s, total in enumerate(table["total"]):
        if sum(r["mass"][s] for r in table["rows"]) != total:
            raise ValueError(f"otu samples table: column mass_{s + 1} does not sum to its total")
    return table


def parse_otu_samples_ppm(text: str) -> dict:
    """the text of PREFIX_otu_samples_ppm.txt -> the same shape, `mass` holding the ppm"""
    table = _parse_otu(text, "otu samples ppm table", lambda x: x.isdigit() and int(x) <= 1000000, int)
    for s in range(len(table["libs"])):
        if sum(r["mass"][s] for r in table["rows"]) > 1000000:
            raise ValueError(f"otu samples ppm table: column mass_{s + 1} sums to more than 10^6")
    return table


def read_otu_samples(path: str) -> dict:
    with open(path, encoding="latin-1") as fh:
        return parse_otu_samples(fh.read())


def read_otu_samples_ppm(path: str) -> dict:
    with open(path, encoding="latin-1") as fh:
        return parse_otu_samples_ppm(fh.read())


def write_otu_samples(prefix: str, samplecov_path: str, clust_path: str) -> dict:
    """PREFIX_otu_samples.txt and PREFIX_otu_samples_ppm.txt from the files of the steps before.  Everything is read and joined first:
    when the tables do not fit each other this raises ValueError and writes nothing.  -> the result of join"""
    from .cluster import read_clust
    table = join(read_samplecov(samplecov_path), read_clust(clust_path))
    texts = (otu_samples_text(table), otu_samples_ppm_text(table))
    for path, text in zip((prefix + "_otu_samples.txt", prefix + "_otu_samples_ppm.txt"), texts):
        with open(path, "w", encoding="latin-1") as fh:
            fh.write(text)
    return table


def main(argv=None) -> int:
    """samplecov.py OUT_PREFIX SAMPLECOV CLUST: the join as a command"""
    a = list(sys.argv[1:] if argv is None else argv)
    if len(a) != 3:
        print("Usage: python -m megagta_amd.samplecov <out_prefix> <x_samplecov.txt> <x_clust.txt>", file=sys.stderr)
        return 2
    try:
        table = write_otu_samples(a[0], a[1], a[2])
    except (ValueError, OSError) as e:
        print("samplecov: " + str(e).removeprefix("samplecov: "), file=sys.stderr)
        return 1
    print("%d clusters x %d libraries, total mass %s" % (sum(r["cluster"] is not None for r in table["rows"]), len(table["libs"]),
                                                        " ".join(e4_text(t) for t in table["total"])), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
