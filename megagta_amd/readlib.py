"""Read-library host logic: `reads.lib.bin` / `.lib_info` <-> the packed, REVERSED read array the
SdBG build consumes.

Formats (reference): per read `uint32 len` + ceil(len/16) 2-bit words, forward orientation
(sequence_manager.cpp:375-410); `.lib_info` = "total_bases num_reads" + 2 lines per library
(read_lib_functions-inl.h:216-225).  `buildgraph` loads every read reversed, not complemented
(cx1_read2sdbg_s1.cpp:97,117) into one contiguous 2-bit array with base j of a word at bits 30-2j
(sequence_package.h:126-129).
"""
from __future__ import annotations

import numpy as np

_SHIFTS = (30 - 2 * np.arange(16)).astype(np.uint32)


def read_lib_info(prefix: str) -> tuple[int, int]:
    with open(prefix + ".lib_info") as f:
        total_bases, num_reads = (int(x) for x in f.readline().split()[:2])
    return total_bases, num_reads


def read_lib_table(prefix: str) -> list:
    """[(text, from, to, max_read_len, is_pe)] per library, from the two lines per library behind the first line of `.lib_info`: the
    library's line of the read_lib file as it stood, then `from to max_read_len pe|se` (read numbers, `to` inclusive: an empty library
    has to = from - 1).  The ranges must tile [0, num_reads) in order; anything else is a ValueError."""
    with open(prefix + ".lib_info", encoding="latin-1") as f:
        lines = f.read().split("\n")
    try:
        num_reads = int(lines[0].split()[1])
    except (IndexError, ValueError):
        raise ValueError(f"{prefix}.lib_info: the first line is not `total_bases num_reads`") from None
    if lines and lines[-1] == "":
        lines.pop()
    if len(lines) % 2 != 1:
        raise ValueError(f"{prefix}.lib_info: a library is two lines, {len(lines) - 1} lines follow the first")
    table, at = [], 0
    for i in range(1, len(lines), 2):
        f = lines[i + 1].split()
        if len(f) != 4 or f[3] not in ("pe", "se") or not all(x.lstrip("-").isdigit() for x in f[:3]):
            raise ValueError(f"{prefix}.lib_info: bad library line {lines[i + 1]!r}")
        frm, to, max_len = int(f[0]), int(f[1]), int(f[2])
        if frm != at or to < frm - 1:
            raise ValueError(f"{prefix}.lib_info: library {len(table) + 1} holds the reads {frm} .. {to}, the libraries before it end at {at}")
        table.append((lines[i], frm, to, max_len, f[3] == "pe"))
        at = to + 1
    if at != num_reads:
        raise ValueError(f"{prefix}.lib_info: the libraries hold {at} reads, the first line says {num_reads}")
    return table


def load_lib_bin(prefix: str) -> list[np.ndarray]:
    """Returns the reads as arrays of base codes (forward orientation)."""
    raw = np.fromfile(prefix + ".bin", dtype=np.uint32)
    _, num_reads = read_lib_info(prefix)
    reads, pos = [], 0
    for _ in range(num_reads):
        ln = int(raw[pos])
        nw = (ln + 15) // 16
        words = raw[pos + 1:pos + 1 + nw]
        codes = ((words[:, None] >> _SHIFTS[None, :]) & 3).astype(np.uint8).reshape(-1)[:ln]
        reads.append(codes)
        pos += 1 + nw
    if pos != raw.size:
        raise ValueError(f"{prefix}.bin: trailing data ({raw.size - pos} words)")
    return reads


def pack_codes(codes: np.ndarray) -> np.ndarray:
    n = codes.size
    nw = (n + 15) // 16
    buf = np.zeros(nw * 16, dtype=np.uint32)
    buf[:n] = codes
    return np.bitwise_or.reduce(buf.reshape(nw, 16) << _SHIFTS[None, :], axis=1).astype(np.uint32)


def pack_for_build(reads: list[np.ndarray]) -> tuple[np.ndarray, np.ndarray]:
    """(packed uint32 words, start_idx uint64[n+1]) with every read reversed."""
    lens = np.array([r.size for r in reads], dtype=np.uint64)
    start = np.zeros(len(reads) + 1, dtype=np.uint64)
    np.cumsum(lens, out=start[1:])
    flat = np.concatenate([r[::-1] for r in reads]) if reads else np.zeros(0, dtype=np.uint8)
    packed = pack_codes(flat)
    if packed.size == 0:
        packed = np.zeros(1, dtype=np.uint32)
    return packed, start


def load_for_build(prefix: str) -> tuple[np.ndarray, np.ndarray]:
    return pack_for_build(load_lib_bin(prefix))
