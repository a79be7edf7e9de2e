"""Phase files: what `megagta.py --pileup --phase` writes from Context.phase (mgta_reads_phase, include/megagta_hip.h).

  PREFIX_phase_links.txt   `#contig pos1 pos2 fragments haplotypes phased` (tabs), one line per tabled pair of sites with fragments =
                           the sum of the pair's 16 cells >= min_link (default 4; a pair without a fragment is never listed), in site
                           order.  Positions are 1-based.  haplotypes = the non-zero cells as `AC:12,GT:9` (the letter at pos1, the
                           letter at pos2), by count descending, then by letters.  phased = 1 iff at least two cells have count * 1000
                           >= min_hap_permille * fragments (default 100) and no two of THOSE cells share the letter at pos1 or the
                           letter at pos2; else 0.
  PREFIX_phase_blocks.txt  `#contig block sites first last positions`: the connected components of a contig's sites under its phased
                           links, those of at least two sites, numbered from 1 per contig by their first position; positions = the
                           1-based positions of the block, ascending, joined by commas.

The counting rule is the library's; this module holds the link rule, the block rule and the writers and readers of the two files.
"""
from __future__ import annotations

import numpy as np

from .pileup import MIN_ALT_PERMILLE, MIN_DEPTH, variant_mask

LINKS_HEADER = "#contig\tpos1\tpos2\tfragments\thaplotypes\tphased\n"
BLOCKS_HEADER = "#contig\tblock\tsites\tfirst\tlast\tpositions\n"
MAX_SPAN, MIN_LINK, MIN_HAP_PERMILLE = 1000, 4, 100
LINK_DTYPE = np.dtype([("contig", "<i8"), ("u", "<i8"), ("v", "<i8"), ("fragments", "<u8"), ("phased", "u1")])   # one tabled pair that is listed
_BASES = "ACGT"


def sites_from_pileup(seqs, res, min_depth: int = MIN_DEPTH, min_alt_permille: int = MIN_ALT_PERMILLE) -> list[np.ndarray]:
    """the positions pileup.variant_mask lists, per contig: the `sites` of Context.phase.  res = what Graph.pileup returned for seqs"""
    off, counts = res["offsets"], res["counts"]
    return [np.flatnonzero(variant_mask(seq, counts[int(off[i]):int(off[i + 1])], min_depth, min_alt_permille)) for i, seq in enumerate(seqs)]


def haplotype_cells(cells) -> list[tuple[str, int]]:
    """the non-zero cells of one pair as (letters, count), by count descending and then by letters"""
    c = [int(x) for x in np.asarray(cells).reshape(16)]
    return sorted(((_BASES[j >> 2] + _BASES[j & 3], c[j]) for j in range(16) if c[j]), key=lambda t: (-t[1], t[0]))


def is_phased(cells, min_hap_permille: int = MIN_HAP_PERMILLE) -> bool:
    hap = haplotype_cells(cells)
    total = sum(n for _, n in hap)
    major = [h for h, n in hap if n * 1000 >= int(min_hap_permille) * total]
    return len(major) >= 2 and len({h[0] for h in major}) == len(major) and len({h[1] for h in major}) == len(major)


def links(res, min_link: int = MIN_LINK, min_hap_permille: int = MIN_HAP_PERMILLE) -> np.ndarray:
    """the listed pairs of a Context.phase result, in site order (LINK_DTYPE: u and v are site numbers of the call)"""
    site_off, pair_off, joint = res["site_off"], res["pair_off"], res["joint"]
    totals = joint.astype(np.uint64).sum(axis=1) if len(joint) else np.zeros(0, dtype=np.uint64)
    out = []
    for i in range(len(site_off) - 1):
        for u in range(int(site_off[i]), int(site_off[i + 1])):
            for p in range(int(pair_off[u]), int(pair_off[u + 1])):
                if int(totals[p]) >= max(1, int(min_link)):
                    out.append((i, u, u + 1 + p - int(pair_off[u]), int(totals[p]), is_phased(joint[p], min_hap_permille)))
    return np.array(out, dtype=LINK_DTYPE)


def blocks(res, link_rows) -> list[tuple[int, list[int]]]:
    """(contig, site numbers ascending) of every connected component of at least two sites under the phased links, by contig and first site"""
    parent = list(range(int(res["site_off"][-1])))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for r in link_rows:
        if r["phased"]:
            a, b = find(int(r["u"])), find(int(r["v"]))
            parent[max(a, b)] = min(a, b)                                      # the root is the component's first site
    out = []
    for i in range(len(res["site_off"]) - 1):
        comp = {}
        for u in range(int(res["site_off"][i]), int(res["site_off"][i + 1])):
            comp.setdefault(find(u), []).append(u)
        out += [(i, members) for root, members in sorted(comp.items()) if len(members) >= 2]
    return out


def format_phase(names, res, min_link: int = MIN_LINK, min_hap_permille: int = MIN_HAP_PERMILLE) -> dict:
    """names of the contigs in the call's order + the dict Context.phase returned -> dict(links=, blocks=): the texts of the two files"""
    if len(names) != len(res["site_off"]) - 1:
        raise ValueError("names and contigs differ in number")
    pos, pair_off, joint = res["site_pos"], res["pair_off"], res["joint"]
    rows = links(res, min_link, min_hap_permille)
    link_text = [LINKS_HEADER]
    for r in rows:
        u, v = int(r["u"]), int(r["v"])
        hap = ",".join(f"{h}:{n}" for h, n in haplotype_cells(joint[int(pair_off[u]) + v - u - 1]))
        link_text.append(f"{names[int(r['contig'])]}\t{int(pos[u]) + 1}\t{int(pos[v]) + 1}\t{int(r['fragments'])}\t{hap}\t{int(r['phased'])}\n")
    block_text, number, last = [BLOCKS_HEADER], 0, -1
    for i, members in blocks(res, rows):
        number = number + 1 if i == last else 1
        last = i
        p = [int(pos[u]) + 1 for u in members]
        block_text.append(f"{names[i]}\t{number}\t{len(p)}\t{p[0]}\t{p[-1]}\t{','.join(str(x) for x in p)}\n")
    return dict(links="".join(link_text), blocks="".join(block_text))


def write_phase(prefix: str, names, res, min_link: int = MIN_LINK, min_hap_permille: int = MIN_HAP_PERMILLE) -> list[str]:
    """-> the paths written"""
    texts = format_phase(names, res, min_link, min_hap_permille)
    paths = []
    for key, suffix in (("links", "_phase_links.txt"), ("blocks", "_phase_blocks.txt")):
        with open(prefix + suffix, "w") as f:
            f.write(texts[key])
        paths.append(prefix + suffix)
    return paths


def parse_links(text: str) -> list[dict]:
    lines = text.splitlines(keepends=True)
    if not lines or lines[0] != LINKS_HEADER:
        raise ValueError("not a phase links file: the header line differs")
    out = []
    for ln in lines[1:]:
        f = ln.rstrip("\n").split("\t")
        if len(f) != 6 or f[5] not in ("0", "1"):
            raise ValueError(f"phase links: bad line {ln!r}")
        hap = [(h.split(":")[0], int(h.split(":")[1])) for h in f[4].split(",")]
        row = dict(contig=f[0], pos1=int(f[1]), pos2=int(f[2]), fragments=int(f[3]), haplotypes=hap, phased=int(f[5]))
        if row["fragments"] != sum(n for _, n in hap) or row["pos1"] >= row["pos2"]:
            raise ValueError(f"phase links: fragments is not the sum of the haplotypes, or pos1 is not below pos2, in {ln!r}")
        out.append(row)
    return out


def parse_blocks(text: str) -> list[dict]:
    lines = text.splitlines(keepends=True)
    if not lines or lines[0] != BLOCKS_HEADER:
        raise ValueError("not a phase blocks file: the header line differs")
    out = []
    for ln in lines[1:]:
        f = ln.rstrip("\n").split("\t")
        if len(f) != 6:
            raise ValueError(f"phase blocks: {len(f)} fields in {ln!r}")
        p = [int(x) for x in f[5].split(",")]
        row = dict(contig=f[0], block=int(f[1]), sites=int(f[2]), first=int(f[3]), last=int(f[4]), positions=p)
        if row["sites"] != len(p) or row["first"] != p[0] or row["last"] != p[-1] or len(p) < 2:
            raise ValueError(f"phase blocks: sites, first or last do not fit the positions in {ln!r}")
        out.append(row)
    return out
