"""The files of `megagta sharecov` and of `megagta.py --taxon-abund`: the writers, the readers and the join that turns the window-shared
coverage of a gene's contigs into an abundance per cluster and per reference organism.  Host only, no device; masses and ppm in integers only.

  PREFIX_sharecov.txt     `#contig<TAB>len<TAB>windows<TAB>covered<TAB>unique<TAB>max_share<TAB>mass`, then one line per FASTA record in
                          file order (mgta_contig_share_coverage over the whole file in one call).  mass is the record's Q16 mass m
                          printed with four decimals: q = m * 10000 >> 16, then q / 10000 `.` q % 10000 -- no floating point, so the
                          C++ host and this module print the same bytes at any size.
  PREFIX_otu_abund.txt    `#cluster<TAB>rep<TAB>contigs<TAB>mass<TAB>ppm<TAB>ref<TAB>identity<TAB>chimera`, one line per cluster in cluster
                          order; a last line `-<TAB>-<TAB>n<TAB>mass<TAB>ppm<TAB>-<TAB>0.0000<TAB>-` for the n > 0 records that are
                          `unaligned` in PREFIX_clust.txt.
  PREFIX_taxon_abund.txt  `#ref<TAB>clusters<TAB>contigs<TAB>mass<TAB>ppm<TAB>lineage`, one line per reference in file order (zeros where
                          nothing is nearest to it), then `#chimeric` and `#unassigned`; only with a nearest table.

From the file on a mass is an integer number of ten-thousandths (the q above): the tables are summed in that unit, so the masses of
both tables add up to the total of PREFIX_sharecov.txt exactly.  ppm = floor(mass * 10^6 / total), 0 when the total is 0; the ppm of a
table are floors and sum to at most 10^6.  The definitions are this project's own.
"""
from __future__ import annotations

import re
import sys

from .align import record_name

SHARECOV_HEADER = "#contig\tlen\twindows\tcovered\tunique\tmax_share\tmass\n"
OTU_HEADER = "#cluster\trep\tcontigs\tmass\tppm\tref\tidentity\tchimera\n"
TAXON_HEADER = "#ref\tclusters\tcontigs\tmass\tppm\tlineage\n"
CHIMERA_WORDS = ("clean", "chimeric", "unchecked", "-")
PSEUDO_REFS = ("#chimeric", "#unassigned")
_MASS = re.compile(r"^(\d+)\.(\d{4})$")
_IDENTITY = re.compile(r"^[01]\.\d{4}$")


def q16_to_e4(mass: int) -> int:
    """a Q16 mass -> ten-thousandths, rounded down"""
    mass = int(mass)
    if not 0 <= mass < 1 << 64:
        raise ValueError(f"mass {mass} is outside 64 bits")
    return (mass * 10000) >> 16


def e4_text(q: int) -> str:
    return "%d.%04d" % divmod(int(q), 10000)


def q16_text(mass: int) -> str:
    """what `megagta sharecov` prints for a Q16 mass"""
    return e4_text(q16_to_e4(mass))


def parse_e4(text: str) -> int:
    m = _MASS.match(text)
    if not m:
        raise ValueError(f"not a mass with four decimals: {text!r}")
    return int(m.group(1)) * 10000 + int(m.group(2))


def ppm_of(mass: int, total: int) -> int:
    return mass * 1000000 // total if total else 0


# ---- PREFIX_sharecov.txt --------------------------------------------------------------------------------------------------------------
def sharecov_text(names, contigs) -> str:
    """names[i] + contigs[i] (a row of Graph.contig_share_coverage()['contigs'], or a dict with len / n_windows / n_covered / n_unique /
    max_share / mass, mass in Q16) -> the text of PREFIX_sharecov.txt"""
    out = [SHARECOV_HEADER]
    for name, c in zip(names, contigs):
        out.append("%s\t%d\t%d\t%d\t%d\t%d\t%s\n" % (name, int(c["len"]), int(c["n_windows"]), int(c["n_covered"]), int(c["n_unique"]), int(c["max_share"]),
                                                     q16_text(int(c["mass"]))))
    return "".join(out)


def parse_sharecov(text: str) -> list:
    """the text of PREFIX_sharecov.txt -> one dict per row in file order: contig str, len / windows / covered / unique / max_share int,
    mass int in ten-thousandths"""
    lines = text.splitlines()
    if not lines or lines[0] + "\n" != SHARECOV_HEADER:
        raise ValueError("sharecov table: the header line is missing")
    rows = []
    for line in lines[1:]:
        f = line.split("\t")
        if len(f) != 7 or not all(x.isdigit() for x in f[1:6]) or not _MASS.match(f[6]):
            raise ValueError(f"sharecov table: bad line {line!r}")
        r = dict(contig=f[0], len=int(f[1]), windows=int(f[2]), covered=int(f[3]), unique=int(f[4]), max_share=int(f[5]), mass=parse_e4(f[6]))
        if r["covered"] > r["windows"] or r["unique"] > r["covered"] or (r["covered"] == 0) != (r["max_share"] == 0) or (r["covered"] == 0 and r["mass"]):
            raise ValueError(f"sharecov table: bad line {line!r}")
        rows.append(r)
    return rows


def read_sharecov(path: str) -> list:
    with open(path, encoding="latin-1") as fh:
        return parse_sharecov(fh.read())


# ---- the references with their descriptions -------------------------------------------------------------------------------------------
def parse_ref_headers(text: str) -> list:
    """[(name, lineage)] of a reference FASTA in file order: name = the header up to the first blank, lineage = the rest of the header
    line behind it, `-` when there is none (megagta_amd.nearest.parse_refs keeps the names only)"""
    out = []
    for line in text.splitlines():
        if line.startswith(">"):
            parts = line[1:].split(None, 1)
            rest = parts[1].strip() if len(parts) > 1 else ""
            out.append((record_name(line[1:]), rest.replace("\t", " ") if rest else "-"))
    return out


def read_ref_headers(path: str) -> list:
    with open(path, encoding="latin-1") as fh:
        return parse_ref_headers(fh.read())


# ---- the join -------------------------------------------------------------------------------------------------------------------------
def _first_index(names) -> dict:
    first = {}
    for i, name in enumerate(names):
        first.setdefault(name, i)
    return first


def join(sharecov, clust, nearest=None, chimera=None, ref_headers=None):
    """sharecov: the rows of parse_sharecov over the nucleotide records; clust: megagta_amd.cluster.parse_clust of the protein records,
    one per nucleotide record, position by position and under the same name; nearest / chimera: megagta_amd.nearest.parse_nearest /
    megagta_amd.chimera.parse_chimera over the representatives, or None where that step did not run; ref_headers: parse_ref_headers of
    the reference file, needed with nearest.  -> (otu rows, taxon rows or None without nearest), masses in ten-thousandths.  Any
    mismatch is a ValueError: nothing is guessed."""
    names = list(clust["names"])
    if len(sharecov) != len(names):
        raise ValueError(f"taxonabund: {len(sharecov)} nucleotide records, {len(names)} lines in the cluster table")
    for i, (r, name) in enumerate(zip(sharecov, names)):
        if r["contig"] != name:
            raise ValueError(f"taxonabund: record {i} is {r['contig']!r} in the nucleotide file and {name!r} in the cluster table")
    if nearest is not None and ref_headers is None:
        raise ValueError("taxonabund: a nearest table needs the reference file it was made from")
    total = sum(r["mass"] for r in sharecov)
    near_at = _first_index(nearest["names"]) if nearest is not None else None
    chim_at = _first_index(chimera["names"]) if chimera is not None else None
    clusters, un_n, un_mass = {}, 0, 0
    for i, r in enumerate(sharecov):
        if int(clust["status"][i]) == 2:
            un_n += 1
            un_mass += r["mass"]
            continue
        c = clusters.setdefault(int(clust["cluster"][i]), dict(rep=names[int(clust["rep"][i])], contigs=0, mass=0))
        if c["rep"] != names[int(clust["rep"][i])]:
            raise ValueError(f"taxonabund: cluster {int(clust['cluster'][i])} has two representatives")
        c["contigs"] += 1
        c["mass"] += r["mass"]
    otu = []
    for number in sorted(clusters):
        c = clusters[number]
        ref, identity, word = None, "0.0000", "-"
        if nearest is not None:
            if c["rep"] not in near_at:
                raise ValueError(f"taxonabund: the representative {c['rep']!r} has no line in the nearest table")
            j = near_at[c["rep"]]
            ref = nearest["ref_names"][j]
            if ref is not None:
                identity = "%.4f" % float(nearest["identity"][j])          # (as the nearest table printed it: four decimals in, four out)
        if chimera is not None:
            if c["rep"] not in chim_at:
                raise ValueError(f"taxonabund: the representative {c['rep']!r} has no line in the chimera table")
            word = CHIMERA_WORDS[int(chimera["recs"][chim_at[c["rep"]]]["status"])]
        otu.append(dict(cluster=number, rep=c["rep"], contigs=c["contigs"], mass=c["mass"], ppm=ppm_of(c["mass"], total), ref=ref, identity=identity, chimera=word))
    if un_n:
        otu.append(dict(cluster=None, rep=None, contigs=un_n, mass=un_mass, ppm=ppm_of(un_mass, total), ref=None, identity="0.0000", chimera="-"))
    if nearest is None:
        return otu, None
    ref_at = _first_index([name for name, _ in ref_headers])
    taxon = [dict(ref=name, clusters=0, contigs=0, mass=0, lineage=lineage) for name, lineage in ref_headers]
    taxon += [dict(ref=name, clusters=0, contigs=0, mass=0, lineage="-") for name in PSEUDO_REFS]
    for row in otu:
        if row["cluster"] is None:                                        # the unaligned records
            t = taxon[-1]
        elif row["chimera"] == "chimeric":
            t = taxon[-2]
        elif row["ref"] is None:
            t = taxon[-1]
        else:
            if row["ref"] not in ref_at:
                raise ValueError(f"taxonabund: the nearest table names {row['ref']!r}, the reference file has no such record")
            t = taxon[ref_at[row["ref"]]]
        t["clusters"] += row["cluster"] is not None
        t["contigs"] += row["contigs"]
        t["mass"] += row["mass"]
    for t in taxon:
        t["ppm"] = ppm_of(t["mass"], total)
    return otu, taxon


# ---- PREFIX_otu_abund.txt and PREFIX_taxon_abund.txt ----------------------------------------------------------------------------------
def otu_text(rows) -> str:
    out = [OTU_HEADER]
    for r in rows:
        out.append("%s\t%s\t%d\t%s\t%d\t%s\t%s\t%s\n" % ("-" if r["cluster"] is None else r["cluster"], r["rep"] or "-", r["contigs"], e4_text(r["mass"]), r["ppm"],
                                                         r["ref"] or "-", r["identity"], r["chimera"]))
    return "".join(out)


def taxon_text(rows) -> str:
    return TAXON_HEADER + "".join("%s\t%d\t%d\t%s\t%d\t%s\n" % (r["ref"], r["clusters"], r["contigs"], e4_text(r["mass"]), r["ppm"], r["lineage"]) for r in rows)


def parse_otu(text: str) -> list:
    """the text of PREFIX_otu_abund.txt -> the rows join made (cluster / rep / ref None where the file has `-`)"""
    lines = text.splitlines()
    if not lines or lines[0] + "\n" != OTU_HEADER:
        raise ValueError("otu table: the header line is missing")
    rows = []
    for n, line in enumerate(lines[1:]):
        f = line.split("\t")
        ok = (len(f) == 8 and (f[0] == "-" or f[0].isdigit()) and f[1] and f[2].isdigit() and _MASS.match(f[3]) and f[4].isdigit() and f[5]
              and _IDENTITY.match(f[6]) and f[7] in CHIMERA_WORDS)
        if ok and f[0] == "-":                                            # the unaligned records: the last line, and nothing but counts
            ok = f[1] == "-" and f[5] == "-" and f[6] == "0.0000" and f[7] == "-" and n == len(lines) - 2 and int(f[2]) > 0
        elif ok:
            ok = f[1] != "-" and int(f[2]) > 0 and (f[5] != "-" or f[6] == "0.0000")
        if not ok or int(f[4]) > 1000000:
            raise ValueError(f"otu table: bad line {line!r}")
        rows.append(dict(cluster=None if f[0] == "-" else int(f[0]), rep=None if f[1] == "-" else f[1], contigs=int(f[2]), mass=parse_e4(f[3]), ppm=int(f[4]),
                         ref=None if f[5] == "-" else f[5], identity=f[6], chimera=f[7]))
    return rows


def parse_taxon(text: str) -> list:
    """the text of PREFIX_taxon_abund.txt -> the rows join made; the two pseudo-references close the table"""
    lines = text.splitlines()
    if not lines or lines[0] + "\n" != TAXON_HEADER:
        raise ValueError("taxon table: the header line is missing")
    rows = []
    for line in lines[1:]:
        f = line.split("\t")
        if len(f) != 6 or not f[0] or not f[1].isdigit() or not f[2].isdigit() or not _MASS.match(f[3]) or not f[4].isdigit() or not f[5] or int(f[4]) > 1000000:
            raise ValueError(f"taxon table: bad line {line!r}")
        r = dict(ref=f[0], clusters=int(f[1]), contigs=int(f[2]), mass=parse_e4(f[3]), ppm=int(f[4]), lineage=f[5])
        if r["clusters"] > r["contigs"] or (r["contigs"] == 0 and r["mass"]):
            raise ValueError(f"taxon table: bad line {line!r}")
        rows.append(r)
    if tuple(r["ref"] for r in rows[-2:]) != PSEUDO_REFS:
        raise ValueError("taxon table: the lines #chimeric and #unassigned are missing at the end")
    return rows


def read_otu(path: str) -> list:
    with open(path, encoding="latin-1") as fh:
        return parse_otu(fh.read())


def read_taxon(path: str) -> list:
    with open(path, encoding="latin-1") as fh:
        return parse_taxon(fh.read())


def write_taxonabund(prefix: str, sharecov_path: str, clust_path: str, nearest_path: str | None = None, chimera_path: str | None = None,
                     refs_path: str | None = None) -> dict:
    """PREFIX_otu_abund.txt and, with a nearest table, PREFIX_taxon_abund.txt from the files of the steps before.  Everything is read and
    joined first: when the tables do not fit each other this raises ValueError and writes nothing.  -> dict(otu, taxon, total)"""
    from .chimera import read_chimera
    from .cluster import read_clust
    from .nearest import read_nearest
    sharecov = read_sharecov(sharecov_path)
    otu, taxon = join(sharecov, read_clust(clust_path), read_nearest(nearest_path) if nearest_path else None,
                      read_chimera(chimera_path) if chimera_path else None, read_ref_headers(refs_path) if refs_path else None)
    with open(prefix + "_otu_abund.txt", "w", encoding="latin-1") as fh:
        fh.write(otu_text(otu))
    if taxon is not None:
        with open(prefix + "_taxon_abund.txt", "w", encoding="latin-1") as fh:
            fh.write(taxon_text(taxon))
    return dict(otu=otu, taxon=taxon, total=sum(r["mass"] for r in sharecov))


def main(argv=None) -> int:
    """taxonabund.py OUT_PREFIX SHARECOV CLUST [NEAREST|- CHIMERA|- REFS|-]: the join as a command"""
    a = list(sys.argv[1:] if argv is None else argv)
    if not 3 <= len(a) <= 6:
        print("Usage: python -m megagta_amd.taxonabund <out_prefix> <x_sharecov.txt> <x_clust.txt> [<x_nearest.txt>|- [<x_chimera.txt>|- [<refs.fasta>|-]]]", file=sys.stderr)
        return 2
    a += ["-"] * (6 - len(a))
    opt = [None if x == "-" else x for x in a[3:]]
    try:
        res = write_taxonabund(a[0], a[1], a[2], *opt)
    except (ValueError, OSError) as e:
        print("taxonabund: " + str(e).removeprefix("taxonabund: "), file=sys.stderr)
        return 1
    print("%d clusters, %d lines per reference, total mass %s" % (sum(r["cluster"] is not None for r in res["otu"]), len(res["taxon"] or ()), e4_text(res["total"])),
          file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
