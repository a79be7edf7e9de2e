"""The files of `megagta cluster` / `megagta.py --cluster`: the writers and the readers, so that tests and users read them one way.
Host only, no device.

  PREFIX_clust.txt        `#contig<TAB>status<TAB>cluster<TAB>rep<TAB>len<TAB>n_diff<TAB>n_overlap`, then one line per input record in
                          input order.  status = rep | member | unaligned; cluster = the cluster's number (clusters are numbered by
                          their lowest record); rep = the name of the cluster's representative; len = the record's residues; n_diff,
                          n_overlap = the record's counts against its representative (the representative itself: 0 and its residue
                          columns).  An unaligned record (no residue in any column of the model) has `-` for cluster and rep, 0 and 0.
  PREFIX_rep_seqs.fasta   the representatives in input order: `>` + the header line as it stood + newline + the A2M line without `-`,
                          upper-cased (ASCII letters only) + newline

`megagta clustertree` / `megagta.py --cluster-dists` write the same two files per cut-off as PREFIX_d<tag>_clust.txt and
PREFIX_d<tag>_rep_seqs.fasta (tag = the cut-off as the user wrote it), and once
  PREFIX_tree.txt         `#a_row<TAB>b_row<TAB>a<TAB>b<TAB>n_diff<TAB>n_overlap`, then one line per merge of the complete-linkage tree up to
                          the largest cut-off, ascending by (n_diff / n_overlap, a_row, b_row): a_row < b_row are the lowest records of the
                          two clusters when they merge, a and b their names, n_diff / n_overlap the distance in lowest terms (0 as 0/1)

The input is PREFIX_aligned.fasta of `megagta align` (megagta_amd/align.py): the row of a record is its A2M line without the
lower-case letters, its length the characters of the line that are not `-`.  The definitions are those of mgta_rows_cluster
(include/megagta_hip.h).
"""
from __future__ import annotations

import numpy as np

from .align import a2m_columns, record_name

STATUS = ("rep", "member", "unaligned")
CLUST_HEADER = "#contig\tstatus\tcluster\trep\tlen\tn_diff\tn_overlap\n"
_UPPER = bytes(range(256)).translate(bytes.maketrans(b"abcdefghijklmnopqrstuvwxyz", b"ABCDEFGHIJKLMNOPQRSTUVWXYZ")).decode("latin-1")


def rows_and_lens(lines):
    """the rows (list of str, all M characters) and the unaligned lengths of A2M lines; a line of another width than the first is an error"""
    rows = [a2m_columns(x) for x in lines]
    for i, r in enumerate(rows):
        if len(r) != len(rows[0]):
            raise ValueError(f"cluster: record {i} has {len(r)} columns, the first record has {len(rows[0])}")
    return rows, np.array([len(x) - x.count("-") for x in lines], dtype=np.int64)


def status_of(i: int, cluster, rep) -> int:
    return 2 if int(cluster[i]) < 0 else (0 if int(rep[i]) == i else 1)


def clust_text(names, lens, result: dict) -> str:
    """the text of PREFIX_clust.txt from the result of Context.cluster over records called `names`, `lens` residues long"""
    cl, rep, rd, ro = result["cluster"], result["rep"], result["rep_diff"], result["rep_overlap"]
    out = [CLUST_HEADER]
    for i, name in enumerate(names):
        s = status_of(i, cl, rep)
        out.append("%s\t%s\t%s\t%s\t%d\t%d\t%d\n" % (name, STATUS[s], "-" if s == 2 else str(int(cl[i])), "-" if s == 2 else names[int(rep[i])], int(lens[i]),
                                                     int(rd[i]), int(ro[i])))
    return "".join(out)


def unaligned_text(line: str) -> str:
    """`to-unaligned-fasta`: an A2M line without `-`, its ASCII letters upper-cased"""
    return line.replace("-", "").translate(_UPPER)


def rep_fasta_text(headers, lines, result: dict) -> str:
    """the text of PREFIX_rep_seqs.fasta: the representatives in input order, from the A2M lines"""
    cl, rep = result["cluster"], result["rep"]
    return "".join(">%s\n%s\n" % (h, unaligned_text(x)) for i, (h, x) in enumerate(zip(headers, lines)) if status_of(i, cl, rep) == 0)


def write_cluster(prefix: str, headers, lines, result: dict, nucl=None, nucl_prefix: str | None = None) -> None:
    """PREFIX_clust.txt and PREFIX_rep_seqs.fasta from the result of Context.cluster over the rows of the A2M `lines`; with nucl =
    [(header, sequence)], one per record and under the same names, also NUCL_PREFIX_rep_seqs.fasta: the representatives' records"""
    names = [record_name(h) for h in headers]
    if nucl is not None:
        if len(nucl) != len(names) or any(record_name(h) != n for (h, _), n in zip(nucl, names)):
            raise ValueError("cluster: the nucleotide records do not carry the names of the aligned records, position by position")
    lens = [len(x) - x.count("-") for x in lines]
    with open(prefix + "_clust.txt", "w", encoding="latin-1") as fh:
        fh.write(clust_text(names, lens, result))
    with open(prefix + "_rep_seqs.fasta", "w", encoding="latin-1") as fh:
        fh.write(rep_fasta_text(headers, lines, result))
    if nucl is not None:
        with open(nucl_prefix + "_rep_seqs.fasta", "w", encoding="latin-1") as fh:
            fh.write("".join(">%s\n%s\n" % (h, s) for i, (h, s) in enumerate(nucl) if status_of(i, result["cluster"], result["rep"]) == 0))


TREE_HEADER = "#a_row\tb_row\ta\tb\tn_diff\tn_overlap\n"


def tree_text(names, merges) -> str:
    """the text of PREFIX_tree.txt from the merges of Context.clusters / Context.pairs_tree (a TREE_MERGE array, or tuples (a, b, n_diff,
    n_overlap)) over records called `names`"""
    rows = merges.tolist() if isinstance(merges, np.ndarray) else [tuple(m) for m in merges]
    return TREE_HEADER + "".join("%d\t%d\t%s\t%s\t%d\t%d\n" % (a, b, names[a], names[b], d, o) for a, b, d, o in rows)


def parse_tree(text: str) -> dict:
    """the text of PREFIX_tree.txt -> dict(merges = [(a_row, b_row, n_diff, n_overlap)], names = {row: name} of the rows the file names)"""
    lines = text.splitlines()
    if not lines or lines[0] + "\n" != TREE_HEADER:
        raise ValueError("tree table: the header line is missing")
    merges, names = [], {}
    for line in lines[1:]:
        f = line.split("\t")
        if len(f) != 6 or not all(f[k].isdigit() for k in (0, 1, 4, 5)):
            raise ValueError(f"tree table: bad line {line!r}")
        a, b, d, o = int(f[0]), int(f[1]), int(f[4]), int(f[5])
        if not (a < b and 1 <= o and d <= o) or names.setdefault(a, f[2]) != f[2] or names.setdefault(b, f[3]) != f[3]:
            raise ValueError(f"tree table: bad line {line!r}")
        merges.append((a, b, d, o))
    return dict(merges=merges, names=names)


def read_tree(path: str) -> dict:
    with open(path, encoding="latin-1") as fh:
        return parse_tree(fh.read())


def write_cluster_tree(prefix: str, headers, lines, tags, result: dict, nucl=None, nucl_prefix: str | None = None) -> None:
    """the files of `megagta clustertree` from the result of Context.clusters over the rows of the A2M `lines`, tags[k] naming cut-off k:
    per tag what write_cluster writes under PREFIX_d<tag> (and NUCL_PREFIX_d<tag>), and PREFIX_tree.txt"""
    if len(tags) != len(result["cluster"]):
        raise ValueError("cluster: one tag per cut-off")
    for k, tag in enumerate(tags):
        one = dict(cluster=result["cluster"][k], rep=result["rep"][k], rep_diff=result["rep_diff"][k], rep_overlap=result["rep_overlap"][k])
        write_cluster(prefix + "_d" + tag, headers, lines, one, nucl, None if nucl_prefix is None else nucl_prefix + "_d" + tag)
    with open(prefix + "_tree.txt", "w", encoding="latin-1") as fh:
        fh.write(tree_text([record_name(h) for h in headers], result["merges"]))


def parse_cutoff_list(text: str):
    """`c1,c2,...` -> (tags, cutoffs): every item is made of 0-9 and `.`, a number in [0, 1]; its text is its tag; two items with the same
    value are an error (ValueError names the item)"""
    tags, cutoffs = [], []
    for item in text.split(","):
        if not item or item.strip("0123456789.") or item.count(".") > 1 or not item.strip("."):
            raise ValueError(f"cut-off {item!r} is not a number in [0, 1] written with 0-9 and .")
        c = float(item)
        if not 0 <= c <= 1:
            raise ValueError(f"cut-off {item!r} is not a number in [0, 1] written with 0-9 and .")
        if c in cutoffs:
            raise ValueError(f"cut-offs {tags[cutoffs.index(c)]!r} and {item!r} are the same number")
        tags.append(item)
        cutoffs.append(c)
    return tags, cutoffs


def parse_clust(text: str) -> dict:
    """the text of PREFIX_clust.txt -> dict(names, status uint8 (0 rep, 1 member, 2 unaligned), cluster int32 (-1 unaligned), rep int64
    (the index of the record rep names first; -1 unaligned), lens int64, rep_diff uint16, rep_overlap uint16)"""
    lines = text.splitlines()
    if not lines or lines[0] + "\n" != CLUST_HEADER:
        raise ValueError("clust table: the header line is missing")
    names, status, cluster, rep_names, lens, rd, ro = [], [], [], [], [], [], []
    for line in lines[1:]:
        f = line.split("\t")
        if len(f) != 7 or f[1] not in STATUS or not all(x.isdigit() for x in f[4:]) or not (f[2] == "-" or f[2].isdigit()):
            raise ValueError(f"clust table: bad line {line!r}")
        s = STATUS.index(f[1])
        if (s == 2) != (f[2] == "-") or (s == 2) != (f[3] == "-"):
            raise ValueError(f"clust table: cluster {f[2]!r} and rep {f[3]!r} do not go with status {f[1]}")
        names.append(f[0]); status.append(s); cluster.append(-1 if s == 2 else int(f[2])); rep_names.append(f[3])
        lens.append(int(f[4])); rd.append(int(f[5])); ro.append(int(f[6]))
    first = {}
    for i, name in enumerate(names):
        first.setdefault(name, i)
    rep = []
    for i, (s, r) in enumerate(zip(status, rep_names)):
        if s != 2 and r not in first:
            raise ValueError(f"clust table: record {i}: no record is called {r!r}")
        if s == 0 and first[r] != first[names[i]]:
            raise ValueError(f"clust table: record {i} is a representative, but of {r!r}")
        rep.append(-1 if s == 2 else (i if s == 0 else first[r]))
    return dict(names=names, status=np.array(status, dtype=np.uint8), cluster=np.array(cluster, dtype=np.int32), rep=np.array(rep, dtype=np.int64),
                lens=np.array(lens, dtype=np.int64), rep_diff=np.array(rd, dtype=np.uint16), rep_overlap=np.array(ro, dtype=np.uint16))


def read_clust(path: str) -> dict:
    with open(path, encoding="latin-1") as fh:
        return parse_clust(fh.read())
