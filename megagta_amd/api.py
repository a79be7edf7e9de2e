"""Python host side above the C ABI: mirrors the reference's `buildgraph` / `search` operator
surface (same inputs, same outputs, same error behaviour) on top of libmegagta_hip.so.

  Context.build_sdbg(...)      <->  `megagta buildgraph`  (build_graph.cpp:33-135)
  write_sdbg(prefix, stream)   <->  SdbgWriter            (sdbg_multi_io.h:34-199)
  read_sdbg(prefix)            <->  SdbgReader            (sdbg_multi_io.h:201-417)
"""
from __future__ import annotations

import ctypes as C
import hashlib
import os
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import MegaGtaError, check
from .recruit import LN2

NUM_BUCKETS = 65536

# the record dtypes of the C ABI (one object each, derived in _lib from the struct's mirror; the stage modules name the same objects:
# align.REC, nearest.REC, chimera.REC, frameshift.REC, recruit.REC, pileup.CONTIG_DTYPE / READ_DTYPE, gapped.PLACE_DTYPE / GAP_DTYPE)
COV_DTYPE, SHARE_DTYPE = _lib.RECORDS[_lib.ContigCov], _lib.RECORDS[_lib.ContigShare]
ALIGN_REC, POST_REC = _lib.RECORDS[_lib.AlignRec], _lib.RECORDS[_lib.PostRec]
ROW_PAIR, TREE_MERGE = _lib.RECORDS[_lib.RowPair], _lib.RECORDS[_lib.TreeMerge]
NEAREST_REC, FRAMESHIFT_REC, CHIMERA_REC = _lib.RECORDS[_lib.NearestRec], _lib.RECORDS[_lib.FrameshiftRec], _lib.RECORDS[_lib.ChimeraRec]
_RECRUIT_REC, _CONTIG_PILEUP = _lib.RECORDS[_lib.RecruitRec], _lib.RECORDS[_lib.ContigPileup]
_READ_PLACE, _GAP_PLACE, _GAP_REC = _lib.RECORDS[_lib.ReadPlace], _lib.RECORDS[_lib.GapPlace], _lib.RECORDS[_lib.GapRec]


@dataclass
class EdgeStream:
    """Logical SdBG edge stream in bucket order (what SdbgWriter::write receives)."""
    k: int
    words_per_tip: int
    bucket_items: np.ndarray                 # int64 [65536] records per bucket
    records: np.ndarray                      # uint16 [num_edges]
    large: np.ndarray                        # uint16 [num_large]
    tips: np.ndarray                         # uint32 [num_tips * words_per_tip]
    bucket_large: np.ndarray = None          # int64 [65536]
    bucket_tips: np.ndarray = None           # int64 [65536]
    stats: dict = field(default_factory=dict)

    def md5(self) -> str:
        h = hashlib.md5()
        h.update(np.int32(self.k).tobytes())
        h.update(self.bucket_items.astype("<i8").tobytes())
        h.update(self.records.astype("<u2").tobytes())
        h.update(self.large.astype("<u2").tobytes())
        h.update(self.tips.astype("<u4").tobytes())
        return h.hexdigest()


# ---- how the wrappers below marshal a call ------------------------------------------------------------------------------------
def _pack(seqs, encoding: str = "utf-8") -> tuple[bytes, np.ndarray, int]:
    """a list of sequences (bytes as they are, anything else by the encoding of its str) -> (the letters back to back, offsets
    uint64[n + 1], n).  The encoding is the call's: the graph and model stages take UTF-8, `nearest`, `frameshift` and `chimera` latin-1."""
    raw = [s if isinstance(s, (bytes, bytearray)) else str(s).encode(encoding) for s in seqs]
    offsets = np.zeros(len(raw) + 1, dtype=np.uint64)
    if raw:
        np.cumsum([len(s) for s in raw], out=offsets[1:])
    return b"".join(raw), offsets, len(raw)


def _window_offsets(offsets: np.ndarray, k: int) -> np.ndarray:
    """int64[n + 1]: the windows in front of every contig, len - k of them per contig and none for a contig of k letters or fewer"""
    woff = np.zeros(len(offsets), dtype=np.int64)
    np.cumsum(np.maximum(0, np.diff(offsets.astype(np.int64)) - k), out=woff[1:])
    return woff


def _known(params: dict | None, names, what: str) -> dict:
    """the call's parameters as a dict; a name the call does not know is an error"""
    unknown = set(params or {}) - set(names)
    if unknown:
        raise ValueError(f"unknown {what} parameters: {sorted(unknown)}")
    return dict(params or {})


def _int_params(cls, params: dict | None, what: str):
    """a *Params struct of integer members from a dict of them; a member that is not named stays 0, the library's word for its default"""
    par = cls()
    for name, v in _known(params, [name for name, _ in cls._fields_], what).items():
        setattr(par, name, int(v))
    return par


def _sub_table(sub) -> np.ndarray:
    table = np.ascontiguousarray(sub, dtype=np.int8)
    if table.shape != (27, 27):
        raise ValueError("sub must be int8[27, 27]")
    return table


def _path_buffers(offsets: np.ndarray, n: int, stride: int) -> tuple[np.ndarray, np.ndarray]:
    """the path letters of n sequences (sequence i writes from offsets[i] + i * stride) and their lengths"""
    return np.zeros(int(offsets[n]) + n * stride + 1, dtype=np.uint8), np.zeros(max(1, n), dtype=np.int32)


def _paths(p: np.ndarray, plen: np.ndarray, offsets: np.ndarray, n: int, stride: int) -> list[str]:
    return [p[int(offsets[i]) + i * stride:int(offsets[i]) + i * stride + int(plen[i])].tobytes().decode() for i in range(n)]


def _one_per_row(lens, n: int) -> np.ndarray:
    ln = np.ascontiguousarray(lens, dtype=np.int64)
    if ln.shape != (n,):
        raise ValueError("lens must hold one length per row")
    return ln


def _residues_and_lens(n_residues, lens) -> tuple[np.ndarray, np.ndarray, int]:
    nr, ln = np.ascontiguousarray(n_residues, dtype=np.int32), np.ascontiguousarray(lens, dtype=np.int64)
    if ln.shape != (nr.size,) or nr.ndim != 1:
        raise ValueError("n_residues and lens must hold one value per row")
    return nr, ln, nr.size


def _linkage_outputs(shape) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """cluster int32, rep int64, rep_diff and rep_overlap uint16 of a linkage"""
    return np.zeros(shape, dtype=np.int32), np.zeros(shape, dtype=np.int64), np.zeros(shape, dtype=np.uint16), np.zeros(shape, dtype=np.uint16)


def _linkage_result(cl, rep, rd, ro, st, **more) -> dict:
    return dict(cluster=cl, rep=rep, rep_diff=rd, rep_overlap=ro, **more, stats=st.as_dict())


def _pair_array(pairs) -> np.ndarray:
    return np.ascontiguousarray(pairs, dtype=ROW_PAIR) if isinstance(pairs, np.ndarray) else np.array([tuple(x) for x in pairs], dtype=ROW_PAIR)


def _hit_bits(words: np.ndarray, ns: int) -> np.ndarray:
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:ns].astype(bool)


class Context:
    """One per GPU (mgta_ctx)."""

    def __init__(self, device: int = 0):
        self._L = _lib.load()
        self.h = self._L.mgta_ctx_create(device)
        if not self.h:
            raise MegaGtaError("mgta_ctx_create failed: " + self._L.mgta_last_error().decode())

    def close(self):
        if getattr(self, "h", None):
            self._L.mgta_ctx_destroy(self.h)
            self.h = None

    __del__ = close

    def set_full_lsd(self, on: int):
        """diagnostic bit mask: 1 = global LSD passes only (no segment-local LDS finish); 2 = LDS finish by LSD passes only (no comparison route)"""
        check(self._L.mgta_ctx_set_full_lsd(self.h, int(on)), "mgta_ctx_set_full_lsd")

    def last_counting(self) -> np.ndarray:
        """(k+1)-mer multiplicity histogram of the last min_count >= 2 build (int64[65536]); `counting_text` renders PREFIX.counting"""
        h = np.zeros(65536, dtype=np.int64)
        check(self._L.mgta_sdbg_last_counting(self.h, h.ctypes.data), "mgta_sdbg_last_counting")
        return h

    def set_mem_limit(self, nbytes: int):
        check(self._L.mgta_ctx_set_mem_limit(self.h, nbytes), "mgta_ctx_set_mem_limit")

    def probe_random_lines(self, table_bytes: int, configs) -> list[dict]:
        """The device's random 128-byte line rate / dependent-line latency (mgta_probe_random_lines).  configs: iterable of
        (waves_per_cu, groups, unroll, dependent, steps); one dict per configuration (lines_in_flight_per_cu, gb_per_s, ns_per_step, ...)."""
        configs = list(configs)
        arr = (_lib.LineProbe * len(configs))()
        for c, (w, g, u, d, steps) in zip(arr, configs):
            c.waves_per_cu, c.groups, c.unroll, c.dependent, c.steps = int(w), int(g), int(u), int(d), int(steps)
        check(self._L.mgta_probe_random_lines(self.h, int(table_bytes), arr, len(configs)), "mgta_probe_random_lines")
        return [c.as_dict() for c in arr]

    def keep_stream(self, on=True):
        """whole-range builds leave their whole edge stream on the device, also when they take several memory-bound passes.  on = 2: and the
        records / tip labels of a pass are not copied to the host for the sink (`detach_stream` brings the whole stream over afterwards)"""
        check(self._L.mgta_ctx_keep_stream(self.h, int(on)), "mgta_ctx_keep_stream")

    def detach_stream(self) -> tuple[np.ndarray, np.ndarray]:
        """the whole edge stream of the last keep-stream build: taken out of the context (mgta_sdbg_stream_detach), downloaded in one piece
        (mgta_stream_download) and freed -> (records uint16, tip label words uint32)"""
        h = C.c_void_p()
        check(self._L.mgta_sdbg_stream_detach(self.h, C.byref(h)), "mgta_sdbg_stream_detach")
        try:
            nr, nt = C.c_uint64(), C.c_uint64()
            check(self._L.mgta_stream_sizes(h, C.byref(nr), C.byref(nt)), "mgta_stream_sizes")
            recs, tips = np.empty(nr.value, dtype=np.uint16), np.empty(nt.value, dtype=np.uint32)
            check(self._L.mgta_stream_download(h, recs.ctypes.data, tips.ctypes.data), "mgta_stream_download")
        finally:
            self._L.mgta_stream_free(h)
        return recs, tips

    def keep_multiplicity(self, on=True):
        """graphs loaded from now on also hold the full multiplicity of every edge (1 byte per edge + the counts above 254): what
        Graph.edge_multiplicity / Graph.contig_coverage need.  Off by default; never implied."""
        check(self._L.mgta_ctx_keep_multiplicity(self.h, int(bool(on))), "mgta_ctx_keep_multiplicity")
        self._keep_multiplicity = bool(on)

    def set_coverage_batch(self, windows: int = 0):
        """windows one batch of Graph.contig_coverage holds in its per-window scratch (0 = the library's 2^29); small values exercise
        the batching on small inputs.  The result does not depend on it."""
        check(self._L.mgta_ctx_set_coverage_batch(self.h, int(windows)), "mgta_ctx_set_coverage_batch")

    def set_share_hash_bits(self, bits: int = 64):
        """bits of the hash the count table of Graph.contig_share_coverage keeps (1 .. 64, default 64); a few bits make nearly every key
        collide and move no output -- a switch for tests"""
        check(self._L.mgta_ctx_set_share_hash_bits(self.h, int(bits)), "mgta_ctx_set_share_hash_bits")

    def set_pileup_chunk(self, reads: int = 0):
        """reads a group of lanes of Graph.pileup takes per visit to the queue head (0 = the library's choice); moves no output -- a
        switch for tests"""
        check(self._L.mgta_ctx_set_pileup_chunk(self.h, int(reads)), "mgta_ctx_set_pileup_chunk")

    def set_phase_chunk(self, slots: int = 0):
        """fragment slots a group of lanes of Context.phase takes per visit to the queue head (0 = the library's choice); moves no
        output -- a switch for tests"""
        check(self._L.mgta_ctx_set_phase_chunk(self.h, int(slots)), "mgta_ctx_set_phase_chunk")

    @staticmethod
    def _site_lists(sites) -> tuple[np.ndarray, np.ndarray]:
        """per contig a list of 0-based positions -> (site_off uint64[n + 1], site_pos uint32[S])"""
        lists = [np.asarray(s, dtype=np.int64).reshape(-1) for s in sites]
        for s in lists:
            if s.size and (int(s.min()) < 0 or int(s.max()) > 0xFFFFFFFF):
                raise ValueError("a site is a position 0 .. 2^32 - 1")
        off = np.zeros(len(lists) + 1, dtype=np.uint64)
        if lists:
            np.cumsum([s.size for s in lists], out=off[1:])
        pos = np.concatenate(lists).astype(np.uint32) if lists else np.zeros(0, dtype=np.uint32)
        return off, np.ascontiguousarray(pos)

    @staticmethod
    def phase_pairs(sites, max_span: int = 0) -> np.ndarray:
        """mgta_phase_pairs (host only, so it needs no context): sites = per contig a list of ascending 0-based positions -> pair_off uint64[S + 1], the number of
        tabled pairs in front of every site; pair (u, v) has the index pair_off[u] + (v - u - 1), pair_off[S] sizes `joint`."""
        off, pos = Context._site_lists(sites)
        pair_off = np.zeros(int(off[-1]) + 1, dtype=np.uint64)
        check(_lib.load().mgta_phase_pairs(off.ctypes.data, pos.ctypes.data if pos.size else None, len(off) - 1, int(max_span), pair_off.ctypes.data), "mgta_phase_pairs")
        return pair_off

    def phase(self, reads: "Reads", place, libs, lens_or_seqs, sites, params: dict | None = None, reads_reversed: bool = True, joint_cap: int | None = None) -> dict:
        """mgta_reads_phase: the alleles of the sites that one fragment shows together, by the rule of include/megagta_hip.h.  place =
        Graph.pileup(..., per_read=True)["reads"] of `reads` against the same contigs; libs = [(lib_end, paired), ...] in read order;
        lens_or_seqs = per contig its length or its letters; sites = per contig a list of ascending 0-based positions; params =
        dict(max_span=), 0 or missing = 1000.  joint_cap (pairs) defaults to what the sites need.  -> dict(site_counts = uint32[S, 4],
        pair_off = uint64[S + 1], joint = uint32[n_pairs, 16], site_off = int64[n + 1], site_pos = uint32[S], stats)."""
        if reads.ctx is not self:
            raise MegaGtaError("mgta_reads_phase: the reads belong to another context")
        lens = [int(x) if isinstance(x, (int, np.integer)) else len(x) for x in lens_or_seqs]
        n = len(lens)
        offsets = np.zeros(n + 1, dtype=np.uint64)
        if n:
            np.cumsum(lens, out=offsets[1:])
        off, pos = self._site_lists(sites)
        if len(off) - 1 != n:
            raise ValueError("sites and contigs differ in number")
        par = _int_params(_lib.PhaseParams, params, "phase")
        ends = np.ascontiguousarray([int(e) for e, _ in libs], dtype=np.uint64)
        paired = np.ascontiguousarray([1 if p else 0 for _, p in libs], dtype=np.uint8)
        pl = np.ascontiguousarray(place, dtype=_READ_PLACE)
        if ends.size and pl.size < int(ends[-1]):
            raise ValueError(f"{pl.size} placement records for {int(ends[-1])} reads")
        S = int(off[-1])
        if joint_cap is None:
            joint_cap = int(self.phase_pairs(sites, par.max_span)[-1])
        counts = np.zeros((S, 4), dtype=np.uint32)
        pair_off = np.zeros(S + 1, dtype=np.uint64)
        joint = np.zeros((int(joint_cap), 16), dtype=np.uint32)
        st = _lib.PhaseStats()
        check(self._L.mgta_reads_phase(reads.h, int(bool(reads_reversed)), pl.ctypes.data if pl.size else None, ends.ctypes.data if ends.size else None,
                                       paired.ctypes.data if paired.size else None, int(ends.size), offsets.ctypes.data, n, off.ctypes.data,
                                       pos.ctypes.data if S else None, C.byref(par), counts.ctypes.data if S else None, pair_off.ctypes.data,
                                       joint.ctypes.data if joint.size else None, int(joint_cap), C.byref(st)), "mgta_reads_phase")
        return dict(site_counts=counts, pair_off=pair_off, joint=joint[:int(pair_off[-1])], site_off=off.astype(np.int64), site_pos=pos, stats=st.as_dict())

    def set_recruit_chunk(self, reads: int = 0):
        """reads a wave of Context.recruit takes per visit to the queue head (0 = the library's choice, at most 64 are taken); moves
        no output -- a switch for tests"""
        check(self._L.mgta_ctx_set_recruit_chunk(self.h, int(reads)), "mgta_ctx_set_recruit_chunk")

    def recruit(self, hmm: "DeviceHmm", reads: "Reads", n_short_reads: int | None = None, params: dict | None = None, recs: bool = True, cols: bool = True,
                reads_reversed: bool = True) -> dict:
        """mgta_reads_recruit: which of the first n_short_reads reads (default: all of `reads`) the model places in one of six frames,
        by the rule of include/megagta_hip.h.  params = dict(min_aa=, min_score= in nats, or min_bits=); missing = 20 residues and 20
        bits.  local=True (or mode=1, MGTA_RECRUIT_LOCAL) scores every stop-free stretch of a frame and in it the best placement of
        any substring; aa_from and aa_len of a record are then the aligned span.  The default is the global rule (mode 0).
        -> dict(hit_bits = uint64[ceil(n / 64)], bits = bool[n], recs = recruit.REC[n] or None, col_depth = uint64[M] or None,
        stats).  Needs no graph."""
        p = _known(params, ("min_aa", "min_score", "min_bits", "local", "mode"), "recruit")
        if "min_score" in p and "min_bits" in p:
            raise ValueError("recruit parameters: min_score (nats) or min_bits, not both")
        if "local" in p and "mode" in p:
            raise ValueError("recruit parameters: local or mode, not both")
        par = _lib.RecruitParams()
        par.min_aa = int(p.get("min_aa", 20))
        par.mode = int(p["mode"]) if "mode" in p else int(bool(p.get("local", False)))
        par.min_score = float(p["min_score"]) if "min_score" in p else float(p.get("min_bits", 20.0)) * LN2
        ns = reads.n_reads if n_short_reads is None else int(n_short_reads)
        words = np.zeros(max(1, (ns + 63) // 64), dtype=np.uint64)          # (never an empty buffer: NULL is an error of its own)
        r = np.zeros(max(1, ns), dtype=_RECRUIT_REC) if recs else None
        depth = np.zeros(max(1, hmm.M), dtype=np.uint64) if cols else None
        st = _lib.RecruitStats()
        check(self._L.mgta_reads_recruit(self.h, hmm.h, reads.h, int(bool(reads_reversed)), ns, C.byref(par), words.ctypes.data, r.ctypes.data if recs else None,
                                         depth.ctypes.data if cols else None, C.byref(st)), "mgta_reads_recruit")
        return dict(hit_bits=words[:(ns + 63) // 64], bits=_hit_bits(words, ns), recs=r[:ns] if recs else None, col_depth=depth[:hmm.M] if cols else None, stats=st.as_dict())

    def set_derep_hash_bits(self, bits: int = 64):
        """bits of both hashes `derep` keeps (1 .. 64, the default): with a few bits nearly every key collides.  The result does not
        depend on it; only stats["n_compares"] does."""
        check(self._L.mgta_ctx_set_derep_hash_bits(self.h, int(bits)), "mgta_ctx_set_derep_hash_bits")

    def derep(self, seqs) -> dict:
        """mgta_seqs_derep: the unique, non-contained sequences of `seqs` (str or bytes, compared byte for byte) -> dict(status =
        uint8[n]: 0 kept, 1 duplicate of an earlier sequence, 2 contained in a longer one; rep = int64[n]: the first occurrence of a
        duplicate, -1 for a contained sequence, itself for a kept one; copies = uint32[n]: inputs equal to a first occurrence, 0 for a
        duplicate; stats).  Needs no graph."""
        buf, offsets, n = _pack(seqs)
        status, rep, copies = np.zeros(max(1, n), dtype=np.uint8), np.zeros(max(1, n), dtype=np.int64), np.zeros(max(1, n), dtype=np.uint32)
        st = _lib.DerepStats()
        check(self._L.mgta_seqs_derep(self.h, buf, offsets.ctypes.data, n, status.ctypes.data, rep.ctypes.data, copies.ctypes.data, C.byref(st)),
              "mgta_seqs_derep")
        return dict(status=status[:n], rep=rep[:n], copies=copies[:n], stats=st.as_dict())

    def set_align_batch(self, cells: int = 0):
        """cells (L * M) of one batch of `align` (0 = the default: by the context's free memory); a batch holds at least one sequence.
        For tests: the result does not depend on it; only stats["n_batches"] does."""
        check(self._L.mgta_ctx_set_align_batch(self.h, int(cells)), "mgta_ctx_set_align_batch")

    def align(self, hmm: "DeviceHmm", seqs, cols: bool = True, paths: bool = False) -> dict:
        """mgta_seqs_align: every sequence of `seqs` (str or bytes) placed on the columns of `hmm` (the rule: include/megagta_hip.h) ->
        dict(recs = structured array [n] with score, status (0 aligned, 1 unaligned), model_from, model_to, n_match, n_insert, n_delete;
        cols = uint8[n, M] when asked for: the upper-cased residue where a match state emitted it, `-` elsewhere; paths = list of str
        over M / I / D when asked for; stats).  Needs no graph."""
        (buf, offsets, n), M = _pack(seqs), hmm.M
        recs = np.zeros(max(1, n), dtype=ALIGN_REC)
        c = np.zeros((max(1, n), M), dtype=np.uint8) if cols else None
        p, plen = _path_buffers(offsets, n, M) if paths else (None, None)
        st = _lib.AlignStats()
        check(self._L.mgta_seqs_align(self.h, hmm.h, buf, offsets.ctypes.data, n, recs.ctypes.data, c.ctypes.data if cols else None,
                                      p.ctypes.data if paths else None, plen.ctypes.data if paths else None, C.byref(st)), "mgta_seqs_align")
        out = dict(recs=recs[:n], stats=st.as_dict())
        if cols:
            out["cols"] = c[:n]
        if paths:
            out["paths"] = _paths(p, plen, offsets, n, M)
        return out

    def set_posterior_batch(self, cells: int = 0):
        """cells (L * M) of one batch of `posterior` (0 = the default: by the context's free memory); a batch holds at least one
        sequence.  For tests: no output depends on it; only stats["n_batches"] and the residency fields do."""
        check(self._L.mgta_ctx_set_posterior_batch(self.h, int(cells)), "mgta_ctx_set_posterior_batch")

    def posterior(self, hmm: "DeviceHmm", seqs, labels=None, cols: bool = True) -> dict:
        """mgta_seqs_posterior: the Forward score of every sequence of `seqs` (str or bytes) on `hmm` and the posteriors of its residues
        (the rule: include/megagta_hip.h) -> dict(recs = structured array [n] with fwd, bwd (nats; -inf when unaligned) and status
        (0 scored, 1 unaligned); pp = list of float64 arrays, one per sequence, when `labels` is given: per residue the posterior of the
        state its label names (+j the match state of node j, -j its insert state, 0 none), `labels` being one sequence of ints per
        sequence (posterior.labels_from_path makes Viterbi's); col_match, col_insert = float64[n, M] when `cols`: the posteriors of
        every match / insert state summed over the residues; stats).  Needs no graph."""
        (buf, offsets, n), M = _pack(seqs), hmm.M
        total = int(offsets[n])
        lab = pp = None
        if labels is not None:
            if len(labels) != n or any(len(l) != int(m) for l, m in zip(labels, np.diff(offsets))):
                raise ValueError("posterior: one label per residue of every sequence")
            lab = np.zeros(total + 1, dtype=np.int32)
            if total:
                lab[:total] = np.concatenate([np.asarray(l, dtype=np.int32).reshape(-1) for l in labels])
            pp = np.zeros(total + 1, dtype=np.float64)
        recs = np.zeros(max(1, n), dtype=POST_REC)
        cm = np.zeros((max(1, n), M), dtype=np.float64) if cols else None
        ci = np.zeros((max(1, n), M), dtype=np.float64) if cols else None
        st = _lib.PostStats()
        check(self._L.mgta_seqs_posterior(self.h, hmm.h, buf, offsets.ctypes.data, n, lab.ctypes.data if lab is not None else None, recs.ctypes.data,
                                          pp.ctypes.data if pp is not None else None, cm.ctypes.data if cols else None, ci.ctypes.data if cols else None,
                                          C.byref(st)), "mgta_seqs_posterior")
        out = dict(recs=recs[:n], stats=st.as_dict())
        if pp is not None:
            out["pp"] = [pp[int(offsets[i]):int(offsets[i + 1])].copy() for i in range(n)]
        if cols:
            out["col_match"], out["col_insert"] = cm[:n], ci[:n]
        return out

    def set_cluster_tile(self, rows: int = 0):
        """rows of one row block of `row_pairs` / `cluster` (0 = the default): the device works on one row block x row block tile at a
        time.  For tests: the result does not depend on it; only stats["n_tiles"] does."""
        check(self._L.mgta_ctx_set_cluster_tile(self.h, int(rows)), "mgta_ctx_set_cluster_tile")

    @staticmethod
    def _rows(rows) -> np.ndarray:
        """uint8[n, M] from an array, or from a list of equally long str / bytes"""
        if isinstance(rows, np.ndarray):
            r = np.ascontiguousarray(rows, dtype=np.uint8)
        else:
            raw = [s if isinstance(s, (bytes, bytearray)) else str(s).encode("latin-1") for s in rows]
            if len({len(s) for s in raw}) > 1:
                raise ValueError("rows must all have the same width")
            r = np.frombuffer(b"".join(raw), dtype=np.uint8).reshape(len(raw), len(raw[0]) if raw else 0)
        if r.ndim != 2:
            raise ValueError("rows must be n x M")
        return r

    def row_pairs(self, rows, min_overlap: int, cutoff: float) -> dict:
        """mgta_rows_pairs: the kept pairs of the aligned rows (the rule: include/megagta_hip.h) -> dict(pairs = structured array with
        i, j, n_diff, n_overlap, sorted by (i, j); stats).  Needs no graph.  One call counts, a second one fills: the all-pairs pass runs
        twice on the device, which is the price of an exactly sized buffer; a caller of the C entry that expects many pairs passes a
        generous buffer at once (`cluster` runs the pass once)."""
        r = self._rows(rows)
        n, M = r.shape
        cnt, st = C.c_int64(0), _lib.ClusterStats()
        check(self._L.mgta_rows_pairs(self.h, r.ctypes.data, n, M, int(min_overlap), float(cutoff), None, 0, C.byref(cnt), C.byref(st)), "mgta_rows_pairs")
        pairs = np.zeros(max(1, cnt.value), dtype=ROW_PAIR)
        if cnt.value:
            got = C.c_int64(0)
            check(self._L.mgta_rows_pairs(self.h, r.ctypes.data, n, M, int(min_overlap), float(cutoff), pairs.ctypes.data, cnt.value, C.byref(got), C.byref(st)),
                  "mgta_rows_pairs")
            if got.value != cnt.value:
                raise MegaGtaError(f"mgta_rows_pairs counted {cnt.value} pairs, then {got.value}")
        return dict(pairs=pairs[:cnt.value], stats=st.as_dict())

    def cluster(self, rows, lens, min_overlap: int, cutoff: float) -> dict:
        """mgta_rows_cluster: complete-linkage clusters of the aligned rows cut at `cutoff` -> dict(cluster = int32[n], -1 for a row
        without residues; rep = int64[n], the row of the cluster's representative (largest lens, lowest index); rep_diff, rep_overlap =
        uint16[n], the counts of a row against its representative; stats).  Needs no graph."""
        r = self._rows(rows)
        n, M = r.shape
        ln = _one_per_row(lens, n)
        cl, rep, rd, ro = _linkage_outputs(max(1, n))
        st = _lib.ClusterStats()
        check(self._L.mgta_rows_cluster(self.h, r.ctypes.data, ln.ctypes.data, n, M, int(min_overlap), float(cutoff), cl.ctypes.data, rep.ctypes.data,
                                        rd.ctypes.data, ro.ctypes.data, C.byref(st)), "mgta_rows_cluster")
        return _linkage_result(cl[:n], rep[:n], rd[:n], ro[:n], st)

    def pairs_tree(self, pairs, n_residues) -> dict:
        """mgta_pairs_tree: the complete-linkage merge tree of the kept pairs of n rows (a ROW_PAIR array ascending by (i, j), or tuples),
        on the device -> dict(merges = TREE_MERGE array: a < b, n_diff / n_overlap in lowest terms, ascending by (fraction, a, b); stats)."""
        p = _pair_array(pairs)
        nr = np.ascontiguousarray(n_residues, dtype=np.int32)
        if nr.ndim != 1:
            raise ValueError("n_residues must hold one value per row")
        n = nr.size
        merges = np.zeros(max(1, n), dtype=TREE_MERGE)
        cnt, st = C.c_int64(0), _lib.TreeStats()
        check(self._L.mgta_pairs_tree(self.h, p.ctypes.data if p.size else None, p.size, nr.ctypes.data, n, merges.ctypes.data, n, C.byref(cnt), C.byref(st)),
              "mgta_pairs_tree")
        return dict(merges=merges[:cnt.value], stats=st.as_dict())

    def clusters(self, rows, lens, min_overlap: int, cutoffs) -> dict:
        """mgta_rows_clusters: the clusters of the aligned rows at every cut-off of `cutoffs` from one pass over the pairs (at the
        largest) and one merge tree -> dict(cluster = int32[n_cutoffs, n], rep = int64[n_cutoffs, n], rep_diff, rep_overlap =
        uint16[n_cutoffs, n]: row k is what `cluster` gives at cutoffs[k]; merges = the tree (TREE_MERGE array); stats)."""
        r = self._rows(rows)
        n, M = r.shape
        ln = _one_per_row(lens, n)
        cut = np.ascontiguousarray(cutoffs, dtype=np.float64)
        if cut.ndim != 1:
            raise ValueError("cutoffs must be a list of numbers")
        k = cut.size
        cl, rep, rd, ro = _linkage_outputs((k, n))                                                    # cut-off j at [j * n, (j + 1) * n)
        merges = np.zeros(max(1, n), dtype=TREE_MERGE)
        cnt, st = C.c_int64(0), _lib.TreeStats()
        check(self._L.mgta_rows_clusters(self.h, r.ctypes.data, ln.ctypes.data, n, M, int(min_overlap), cut.ctypes.data if k else None, k, cl.ctypes.data,
                                         rep.ctypes.data, rd.ctypes.data, ro.ctypes.data, merges.ctypes.data, C.byref(cnt), C.byref(st)), "mgta_rows_clusters")
        return _linkage_result(cl, rep, rd, ro, st, merges=merges[:cnt.value])

    def set_nearest_batch(self, cells: int = 0):
        """cells (L * R) of one trace batch of `nearest` (0 = the default: by the context's free memory); a batch holds at least one
        pair.  For tests: the result does not depend on it; only stats["n_batches"] does."""
        check(self._L.mgta_ctx_set_nearest_batch(self.h, int(cells)), "mgta_ctx_set_nearest_batch")

    def nearest(self, seqs, refs, sub, gap_open: int, gap_extend: int, scores: bool = False, paths: bool = False) -> dict:
        """mgta_seqs_nearest: for every contig of `seqs` (str or bytes) the closest sequence of `refs` (the rule: include/megagta_hip.h);
        sub = int8[27, 27] over the residue classes (0 = no letter, 1 .. 26 = A .. Z) -> dict(recs = structured array [n] with status
        (0 aligned, 1 unaligned), ref (-1 unaligned), score, ref_from, ref_to, n_match, n_ident, n_insert, n_delete; scores =
        int32[n, n_ref] of every pair when asked for, INT32_MIN where a pair has no score; paths = list of str over M / I / D when
        asked for; stats).  Needs no graph."""
        return self._closest("mgta_seqs_nearest", NEAREST_REC, _lib.NearestStats, seqs, refs, sub, (gap_open, gap_extend), scores, paths)

    def frameshift(self, nucl, refs, sub, gap_open: int, gap_extend: int, frameshift: int, scores: bool = False, paths: bool = False) -> dict:
        """mgta_seqs_frameshift: for every NUCLEOTIDE contig of `nucl` (str or bytes) the closest protein of `refs`, with shifts of the
        reading frame by one nucleotide at the cost `frameshift` (the rule: include/megagta_hip.h); sub, gap_open, gap_extend as for
        `nearest` -> dict(recs = structured array [n] (frameshift.REC) with status, ref, score, ref_from, ref_to, n_match, n_ident,
        n_insert, n_delete, n_short, n_long; scores = int32[n, n_ref] when asked for, INT32_MIN where a pair has no score; paths =
        list of str over M / < / > / I / D when asked for; stats).  `set_nearest_batch` sets this call's trace batch too.  Needs no
        graph."""
        return self._closest("mgta_seqs_frameshift", FRAMESHIFT_REC, _lib.FrameshiftStats, nucl, refs, sub, (gap_open, gap_extend, frameshift), scores, paths)

    def _closest(self, entry: str, rec: np.dtype, stats, seqs, refs, sub, costs: tuple, scores: bool, paths: bool) -> dict:
        """`nearest` and `frameshift`: the two C entries take the same arguments but for the costs (two, or three with the frame shift)
        and their own record and stats structs"""
        buf, offsets, n = _pack(seqs, "latin-1")
        rbuf, roffsets, n_ref = _pack(refs, "latin-1")
        table = _sub_table(sub)
        recs = np.zeros(max(1, n), dtype=rec)
        sc = np.zeros((n, n_ref), dtype=np.int32) if scores else None
        p, plen = _path_buffers(offsets, n, 4096) if paths else (None, None)
        st = stats()
        check(getattr(self._L, entry)(self.h, buf, offsets.ctypes.data, n, rbuf, roffsets.ctypes.data, n_ref, table.ctypes.data, *(int(c) for c in costs),
                                      recs.ctypes.data, sc.ctypes.data if scores and sc.size else None, p.ctypes.data if paths else None,
                                      plen.ctypes.data if paths else None, C.byref(st)), entry)
        out = dict(recs=recs[:n], stats=st.as_dict())
        if scores:
            out["scores"] = sc
        if paths:
            out["paths"] = _paths(p, plen, offsets, n, 4096)
        return out

    def set_chimera_segment(self, columns: int = 0):
        """reference columns of one segment of `chimera`'s run, cut at reference boundaries (0 = the library's choice; 1 = one reference
        per segment).  For tests: the result does not depend on it; only stats["n_segments"] and stats["n_groups"] do."""
        check(self._L.mgta_ctx_set_chimera_segment(self.h, int(columns)), "mgta_ctx_set_chimera_segment")

    def set_chimera_groups(self, groups: int = 0):
        """work items a (contig, direction) of `chimera` is cut into, each a run of consecutive segments, at most one per segment (0 =
        the default: one unless the contigs are too few to fill the device).  For tests: the result does not depend on it; only
        stats["n_groups"] and stats["n_items"] do."""
        check(self._L.mgta_ctx_set_chimera_groups(self.h, int(groups)), "mgta_ctx_set_chimera_groups")

    def chimera(self, seqs, refs, sub, gap_open: int, gap_extend: int, min_seg: int, min_gain: int, tops: bool = False) -> dict:
        """mgta_seqs_chimera: for every contig of `seqs` (str or bytes) whether two sequences of `refs` explain it better than one (the
        rule: include/megagta_hip.h); sub, gap_open, gap_extend as for `nearest` -> dict(recs = structured array [n] with status (0
        clean, 1 chimeric, 2 unchecked), ref, score, brk, left_ref, left_score, right_ref, right_score, two, one, gain; tops = a list
        of int32[L, 8] per contig when asked for: P1.score, P1.ref, P2.score, P2.ref, S1.score, S1.ref, S2.score, S2.ref of every row,
        INT32_MIN, -1 where absent; stats).  Needs no graph."""
        buf, offsets, n = _pack(seqs, "latin-1")
        rbuf, roffsets, n_ref = _pack(refs, "latin-1")
        table = _sub_table(sub)
        recs = np.zeros(max(1, n), dtype=CHIMERA_REC)
        tp = np.zeros((int(offsets[n]) + 1, 8), dtype=np.int32) if tops else None
        st = _lib.ChimeraStats()
        check(self._L.mgta_seqs_chimera(self.h, buf, offsets.ctypes.data, n, rbuf, roffsets.ctypes.data, n_ref, table.ctypes.data,
                                        int(gap_open), int(gap_extend), int(min_seg), int(min_gain), recs.ctypes.data, tp.ctypes.data if tops else None,
                                        C.byref(st)), "mgta_seqs_chimera")
        out = dict(recs=recs[:n], stats=st.as_dict())
        if tops:
            out["tops"] = [tp[int(offsets[i]):int(offsets[i + 1])] for i in range(n)]
        return out

    def release_scratch(self):
        """free the work memory kept between calls (build pool, search pool)"""
        check(self._L.mgta_ctx_release_scratch(self.h), "mgta_ctx_release_scratch")

    def set_search_arena(self, log2_base_nodes: int = 0, pool_bytes: int = 0):
        """work memory of the A* searches: base arena of 1 << log2_base_nodes nodes per search slot (0 = default), pool the searches
        grow into (0 = auto).  Small values exercise the in-place growth on small inputs."""
        check(self._L.mgta_ctx_set_search_arena(self.h, int(log2_base_nodes), int(pool_bytes)), "mgta_ctx_set_search_arena")

    def set_search_page_limit(self, pages: int = 0):
        """pages of 2 MB one array of a search (nodes, heap, hash table) may hold beyond its base arena before the search ends as a failed
        side (mgta_astar_stats.n_over_limit): 1 .. 1024, 0 = the library's 1024.  Small values exercise that limit on small inputs."""
        check(self._L.mgta_ctx_set_search_page_limit(self.h, int(pages)), "mgta_ctx_set_search_page_limit")

    def set_search_share(self, num: int = 1, den: int = 1):
        """the search batches that run on this context (astar_search(..., run=this)) take num / den of the CUs, 1 <= num <= den (1 / 1 =
        all of them): what two contexts that search one graph side by side set to 1 / 2 each.  The result does not depend on it."""
        check(self._L.mgta_ctx_set_search_share(self.h, int(num), int(den)), "mgta_ctx_set_search_share")

    # ---- SdBG build ---------------------------------------------------------------------------
    def upload_reads(self, packed: np.ndarray, start_idx: np.ndarray) -> "Reads":
        packed = np.ascontiguousarray(packed, dtype=np.uint32)
        start_idx = np.ascontiguousarray(start_idx, dtype=np.uint64)
        out = C.c_void_p()
        check(self._L.mgta_reads_upload(self.h, packed.ctypes.data, packed.size, start_idx.ctypes.data, start_idx.size - 1,
                                        C.byref(out)), "mgta_reads_upload")
        return Reads(self, out, start_idx.size - 1)

    def adopt_reads(self, d_packed_ptr: int, n_words: int, d_start_ptr: int, n_reads: int, keepalive=None) -> "Reads":
        out = C.c_void_p()
        check(self._L.mgta_reads_adopt_device(self.h, d_packed_ptr, n_words, d_start_ptr, n_reads, C.byref(out)),
              "mgta_reads_adopt_device")
        r = Reads(self, out, n_reads)
        r._keep = keepalive
        return r

    def build_sdbg(self, reads: "Reads", k: int, min_count: int = 1, need_mercy: bool = False, collect: bool = True,
                   n_short_reads: int | None = None, bucket_range: tuple[int, int] = (0, NUM_BUCKETS)) -> EdgeStream:
        """Reads resident on the device -> edge stream (collect=False keeps it on the device: timing runs)."""
        wpt = (2 * k + 31) // 32
        recs, large, tips = [], [], []
        counts = np.zeros((NUM_BUCKETS, 3), dtype=np.int64)

        def sink(user, b0, b1, bc, r, nr, lg, nl, tp, ntw):
            nb = b1 - b0
            counts[b0:b1] = np.ctypeslib.as_array(bc, shape=(nb * 3,)).reshape(nb, 3)
            recs.append(np.ctypeslib.as_array(r, shape=(nr,)).copy() if nr and r else np.zeros(0, np.uint16))     # (NULL: keep_stream(2))
            large.append(np.ctypeslib.as_array(lg, shape=(nl,)).copy() if nl else np.zeros(0, np.uint16))
            tips.append(np.ctypeslib.as_array(tp, shape=(ntw,)).copy() if ntw and tp else np.zeros(0, np.uint32))
            return 0

        cb = _lib.EDGE_SINK(sink) if collect else C.cast(None, _lib.EDGE_SINK)
        st = _lib.BuildStats()
        ns = reads.n_reads if n_short_reads is None else n_short_reads
        check(self._L.mgta_sdbg_build_resident(self.h, reads.h, ns, k, min_count, int(need_mercy), bucket_range[0], bucket_range[1],
                                               cb, None, C.byref(st)),
              "mgta_sdbg_build_resident")
        cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dt)
        stats = st.as_dict()
        fused = C.c_int64(0)                   # (kept out of mgta_build_stats: the struct's layout stays)
        check(self._L.mgta_sdbg_last_emit_fused(self.h, C.byref(fused)), "mgta_sdbg_last_emit_fused")
        stats["n_emit_fused"] = fused.value
        return EdgeStream(k=k, words_per_tip=wpt, bucket_items=counts[:, 0].copy(), records=cat(recs, np.uint16),
                          large=cat(large, np.uint16), tips=cat(tips, np.uint32), bucket_large=counts[:, 1].copy(),
                          bucket_tips=counts[:, 2].copy(), stats=stats)


def export_records_to_torch(ctx: "Context"):
    """records the last build left on the device (its last pass; every pass with Context.keep_stream) as a torch uint8 CUDA tensor:
    device -> device copy, no host round trip"""
    import torch
    n = C.c_uint64()
    check(ctx._L.mgta_sdbg_export_records_device(ctx.h, None, 0, C.byref(n)), "mgta_sdbg_export_records_device")
    t = torch.empty(max(1, n.value * 2), dtype=torch.uint8, device="cuda")
    check(ctx._L.mgta_sdbg_export_records_device(ctx.h, t.data_ptr(), t.numel(), C.byref(n)), "mgta_sdbg_export_records_device")
    return t[: n.value * 2]


class _multiplicity:
    """the context's keep-multiplicity switch set for one load and put back afterwards; .on = what holds during the load"""

    def __init__(self, ctx: "Context", on: bool):
        self.ctx, self.was = ctx, getattr(ctx, "_keep_multiplicity", False)
        self.on = bool(on) or self.was

    def __enter__(self):
        if self.on != self.was:
            self.ctx.keep_multiplicity(self.on)
        return self

    def __exit__(self, *exc):
        if self.on != self.was:
            self.ctx.keep_multiplicity(self.was)
        return False


class Graph:
    """Device-resident succinct de Bruijn graph (mgta_sdbg) <-> SuccinctDBG (succinct_dbg.h:32-247)."""

    def __init__(self, ctx: Context, stream: "EdgeStream | None", k: int = 0, keep_multiplicity: bool = False):
        """stream = None: the edge stream the last build of `ctx` left on the device (mgta_sdbg_load_resident; k = that build's k).
        keep_multiplicity: this load keeps the full edge multiplicities (the context's switch is set for the load and put back; for a
        resident stream of several passes it must also have been on during the build, Context.keep_multiplicity)."""
        if stream is None:
            self.ctx, self.k = ctx, k
            out = C.c_void_p()
            with _multiplicity(ctx, keep_multiplicity) as sw:
                self.keep_multiplicity = sw.on
                check(ctx._L.mgta_sdbg_load_resident(ctx.h, C.byref(out)), "mgta_sdbg_load_resident")
            self.h = out
            self.size = ctx._L.mgta_sdbg_size(self.h)
            self.k = ctx._L.mgta_sdbg_k(self.h)                 # (the build's k, whatever the caller passed)
            return
        self.ctx, self.k = ctx, stream.k
        recs = np.ascontiguousarray(stream.records, dtype=np.uint16)
        bi = np.ascontiguousarray(stream.bucket_items, dtype=np.int64)
        tips = np.ascontiguousarray(stream.tips, dtype=np.uint32)
        out = C.c_void_p()
        with _multiplicity(ctx, keep_multiplicity) as sw:
            self.keep_multiplicity = sw.on
            if sw.on:
                large = np.ascontiguousarray(stream.large, dtype=np.uint16)
                check(ctx._L.mgta_sdbg_load_large(ctx.h, stream.k, recs.ctypes.data, recs.size, bi.ctypes.data, tips.ctypes.data, tips.size,
                                                  stream.words_per_tip, large.ctypes.data, large.size, C.byref(out)), "mgta_sdbg_load_large")
            else:
                check(ctx._L.mgta_sdbg_load(ctx.h, stream.k, recs.ctypes.data, recs.size, bi.ctypes.data, tips.ctypes.data, tips.size,
                                            stream.words_per_tip, C.byref(out)), "mgta_sdbg_load")
        self.h = out
        self.size = ctx._L.mgta_sdbg_size(self.h)

    @classmethod
    def from_files(cls, ctx: Context, prefix: str, keep_multiplicity: bool = False) -> "Graph":
        """PREFIX.sdbg_info + PREFIX.sdbg.* -> graph on the device (mgta_sdbg_load_files: the records are parsed on the device)"""
        self = cls.__new__(cls)
        self.ctx = ctx
        out = C.c_void_p()
        with _multiplicity(ctx, keep_multiplicity) as sw:
            self.keep_multiplicity = sw.on
            check(ctx._L.mgta_sdbg_load_files(ctx.h, os.fsencode(prefix), C.byref(out)), "mgta_sdbg_load_files")
        self.h = out
        self.size = ctx._L.mgta_sdbg_size(self.h)
        self.k = ctx._L.mgta_sdbg_k(self.h)
        return self

    def outgoing(self, edges) -> tuple[np.ndarray, np.ndarray]:
        """OutgoingEdges (succinct_dbg.cpp:78-97) for a batch: (outdeg int8[n], out int64[n,4])"""
        e = np.ascontiguousarray(edges, dtype=np.int64)
        out = np.empty((e.size, 4), dtype=np.int64)
        deg = np.empty(e.size, dtype=np.int8)
        check(self.ctx._L.mgta_sdbg_outgoing(self.h, e.ctypes.data, e.size, out.ctypes.data, deg.ctypes.data), "mgta_sdbg_outgoing")
        return deg, out

    NAV_OPS = {"rank_last": 0, "rank_tip": 1, "rank_w": 2, "select_last": 3, "select_w": 4, "forward": 5, "backward": 6, "last_index": 7,
               "outgoing": 8, "incoming": 9, "prev_simple": 10, "next_simple": 11, "reverse_complement": 12, "label": 13, "out_fd": 14}
    NAV_WIDTH = {"outgoing": 5, "incoming": 5, "out_fd": 29}
    NAV_UNTOUCHED, NAV_UNDEFINED = -2, -3

    def navigate(self, op: str, arg0, arg1=None, arg2=None):
        """mgta_sdbg_navigate: the device navigation function `op` (a key of NAV_OPS) on a batch of argument tuples (include/megagta_hip.h
        has the table: arg0 = position, rank or edge id; arg1 = the symbol of rank_w / select_w, a scalar or one per tuple, or r of an
        out_fd descriptor; arg2 = the descriptor's hint, -1 = none).  -> int64[n] for the one-value operations, int64[n, 5] for outgoing /
        incoming, int64[n, 29] for out_fd, uint8[n, k] symbols 1..4 for label."""
        a0 = np.ascontiguousarray(arg0, dtype=np.int64).reshape(-1)
        n = a0.size
        full = lambda a: None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.int64), (n,)))
        a1, a2 = full(arg1), full(arg2)
        width = self.NAV_WIDTH.get(op, 1)
        out = np.full((n, width), self.NAV_UNTOUCHED, dtype=np.int64)
        sym = np.zeros((n, self.k), dtype=np.uint8) if op == "label" else None
        ptr = lambda a: None if a is None else a.ctypes.data
        check(self.ctx._L.mgta_sdbg_navigate(self.h, self.NAV_OPS[op], ptr(a0), ptr(a1), ptr(a2), n, ptr(out), ptr(sym)), "mgta_sdbg_navigate")
        if op == "label":
            return sym
        return out[:, 0].copy() if width == 1 else out

    def index_edges(self, kmers: list[str]) -> np.ndarray:
        """IndexBinarySearchEdge (succinct_dbg.cpp:530-549) of (k+1)-mers; -1 = absent"""
        m = {"A": 1, "C": 2, "G": 3, "T": 4, "N": 3}
        seqs = np.array([[m.get(c, 0) for c in s.upper()[: self.k + 1]] for s in kmers], dtype=np.uint8).reshape(len(kmers), self.k + 1)
        ids = np.empty(len(kmers), dtype=np.int64)
        check(self.ctx._L.mgta_sdbg_index_edges(self.h, seqs.ctypes.data, len(kmers), ids.ctypes.data), "mgta_sdbg_index_edges")
        return ids

    def invalid_bits(self) -> np.ndarray:
        """the validity bits as they are now (bit e of word e // 64 set = edge e is not part of the graph)"""
        out = np.zeros((self.size + 63) // 64, dtype=np.uint64)
        check(self.ctx._L.mgta_sdbg_invalid_bits(self.h, out.ctypes.data), "mgta_sdbg_invalid_bits")
        return out

    def edge_multiplicity(self, ids) -> np.ndarray:
        """EdgeMultiplicity (succinct_dbg.h:133-147) for a batch of edge ids -> uint16[n]; needs keep_multiplicity=True at the load"""
        e = np.ascontiguousarray(ids, dtype=np.int64)
        out = np.empty(e.size, dtype=np.uint16)
        check(self.ctx._L.mgta_sdbg_edge_multiplicity(self.h, e.ctypes.data, e.size, out.ctypes.data), "mgta_sdbg_edge_multiplicity")
        return out

    def contig_coverage(self, seqs, per_window: bool = False, abundance: bool = True) -> dict:
        """mgta_contig_coverage for a list of contigs (str or bytes, any case): the coverage of a window = the multiplicity of its
        (k+1)-mer's edge, 0 when absent or not ACGT.  -> dict(contigs = structured array (sum, len, n_windows, n_covered, min, max,
        median: the lower median over all windows), abundance = int64[65536] distinct edges per multiplicity over THIS call,
        stats, and with per_window=True per_window = uint16 coverages back to back + window_offsets int64[n + 1]).
        One call = one set of contigs (abundance marks live for one call): pass a gene's contigs together."""
        buf, offsets, n = _pack(seqs)
        cov = np.zeros(n, dtype=COV_DTYPE)
        woff = _window_offsets(offsets, self.ctx._L.mgta_sdbg_k(self.h))                               # (the graph's own k sizes the buffers)
        pw = np.zeros(int(woff[-1]), dtype=np.uint16) if per_window else None
        ab = np.zeros(65536, dtype=np.int64) if abundance else None
        st = _lib.CoverageStats()
        check(self.ctx._L.mgta_contig_coverage(self.h, buf, offsets.ctypes.data, n, cov.ctypes.data if n else None,
                                               pw.ctypes.data if per_window and pw.size else None, ab.ctypes.data if abundance else None,
                                               C.byref(st)), "mgta_contig_coverage")
        out = dict(contigs=cov, abundance=ab, stats=st.as_dict())
        if per_window:
            out["per_window"], out["window_offsets"] = pw, woff
        return out

    def contig_share_coverage(self, seqs, per_window: bool = False) -> dict:
        """mgta_contig_share_coverage for a list of contigs (str or bytes, any case): the multiplicity of every edge split among the windows
        of THIS call that land on it, so that the masses add up over any set of contigs.  -> dict(contigs = structured array (mass: Q16,
        len, n_windows, n_covered, n_unique, max_share), stats, and with per_window=True per_window_share = uint32 shares back to back
        (0 = no edge), per_window = uint16 multiplicities + window_offsets int64[n + 1]).  One call = one set of contigs."""
        buf, offsets, n = _pack(seqs)
        rec = np.zeros(n, dtype=SHARE_DTYPE)
        woff = _window_offsets(offsets, self.ctx._L.mgta_sdbg_k(self.h))                               # (the graph's own k sizes the buffers)
        pws = np.zeros(int(woff[-1]), dtype=np.uint32) if per_window else None
        pw = np.zeros(int(woff[-1]), dtype=np.uint16) if per_window else None
        st = _lib.ShareStats()
        check(self.ctx._L.mgta_contig_share_coverage(self.h, buf, offsets.ctypes.data, n, rec.ctypes.data if n else None,
                                                     pws.ctypes.data if per_window and pws.size else None, pw.ctypes.data if per_window and pw.size else None,
                                                     C.byref(st)), "mgta_contig_share_coverage")
        out = dict(contigs=rec, stats=st.as_dict(), per_window_share=pws, per_window=pw)
        if per_window:
            out["window_offsets"] = woff
        return out

    def match_reads(self, reads: "Reads", seqs, n_short_reads: int | None = None, counts: bool = False, reads_reversed: bool = True) -> dict:
        """mgta_reads_match_contigs: which of the first n_short_reads reads (default: all of `reads`) share a (k+1)-mer with the contigs
        `seqs` (str or bytes, any case), on either strand.  -> dict(bits = bool[n_short_reads], hit_windows = None, or with counts=True
        uint32[n_short_reads] hitting windows per read, stats).  Without counts the walk of a read ends at its first hit.  Any loaded
        graph will do (no multiplicities needed); one call = one set of contigs."""
        buf, offsets, n = _pack(seqs)
        ns = reads.n_reads if n_short_reads is None else int(n_short_reads)
        words = np.zeros(max(1, (ns + 63) // 64), dtype=np.uint64)          # (never an empty buffer: NULL is an error of its own)
        hits = np.zeros(ns, dtype=np.uint32) if counts else None
        st = _lib.MatchStats()
        check(self.ctx._L.mgta_reads_match_contigs(self.h, reads.h, int(bool(reads_reversed)), ns, buf, offsets.ctypes.data, n, words.ctypes.data,
                                                   hits.ctypes.data if counts and ns else None, C.byref(st)), "mgta_reads_match_contigs")
        return dict(bits=_hit_bits(words, ns), hit_windows=hits, stats=st.as_dict())

    def contig_sample_coverage(self, reads: "Reads", lib_end, seqs, per_window: bool = False, reads_reversed: bool = True) -> dict:
        """mgta_contig_sample_coverage: the read windows of every library on the windows of the contigs `seqs` (str or bytes, any case),
        counted from the reads on either strand and split among the windows of THIS call on one edge.  Library s holds the reads
        [lib_end[s - 1], lib_end[s]) of `reads`; what lies behind lib_end[-1] is not scanned.  -> dict(mass = uint64[n, n_libs] (Q16),
        contigs = structured array as of contig_share_coverage (mass = the sum over the libraries), lib_hit_windows = uint64[n_libs],
        stats, and with per_window=True per_window_count = uint64[windows, n_libs], per_window_share = uint32[windows] (0 = no edge) +
        window_offsets int64[n + 1]).  Any loaded graph will do; one call = one set of contigs."""
        buf, offsets, n = _pack(seqs)
        ends = np.ascontiguousarray(lib_end, dtype=np.uint64)
        if ends.ndim != 1:
            raise ValueError("lib_end is a list of read numbers")
        nl = int(ends.size)
        rec = np.zeros(n, dtype=SHARE_DTYPE)
        woff = _window_offsets(offsets, self.ctx._L.mgta_sdbg_k(self.h))                               # (the graph's own k sizes the buffers)
        mass = np.zeros((n, nl), dtype=np.uint64)
        hits = np.zeros(max(1, nl), dtype=np.uint64)
        pwc = np.zeros((int(woff[-1]), nl), dtype=np.uint64) if per_window else None
        pws = np.zeros(int(woff[-1]), dtype=np.uint32) if per_window else None
        keep = np.zeros(1, dtype=np.uint64)                                    # (never a NULL mass for n = 0: NULL is an error of its own)
        st = _lib.SampleCovStats()
        check(self.ctx._L.mgta_contig_sample_coverage(self.h, reads.h, int(bool(reads_reversed)), ends.ctypes.data if nl else None, nl, buf,
                                                      offsets.ctypes.data, n, mass.ctypes.data if mass.size else keep.ctypes.data, rec.ctypes.data if n else None,
                                                      pwc.ctypes.data if per_window and pwc.size else None, pws.ctypes.data if per_window and pws.size else None,
                                                      hits.ctypes.data, C.byref(st)), "mgta_contig_sample_coverage")
        out = dict(mass=mass, contigs=rec, lib_hit_windows=hits[:nl], stats=st.as_dict(), per_window_count=pwc, per_window_share=pws)
        if per_window:
            out["window_offsets"] = woff
        return out

    def pileup(self, reads: "Reads", seqs, n_short_reads: int | None = None, params: dict | None = None, per_read: bool = False,
               reads_reversed: bool = True) -> dict:
        """mgta_reads_pileup: the first n_short_reads reads (default: all of `reads`) placed on the contigs `seqs` (str or bytes, any
        case) by the rule of include/megagta_hip.h.  params = dict(min_anchors=, min_overlap=, max_mismatch_permille=), 0 or missing =
        the default of each.  -> dict(counts = uint32[letters, 4] (A C G T, in the contig's strand), uniq = uint32[letters], contigs =
        structured array (pileup.CONTIG_DTYPE), offsets = int64[n + 1], stats, and with per_read=True reads = structured array
        (pileup.READ_DTYPE) of n_short_reads records).  Any loaded graph will do; one call = one set of contigs."""
        buf, offsets, n = _pack(seqs)
        ns = reads.n_reads if n_short_reads is None else int(n_short_reads)
        total = int(offsets[-1])
        counts = np.zeros((total, 4), dtype=np.uint32)
        uniq = np.zeros(total, dtype=np.uint32)
        rec = np.zeros(n, dtype=_CONTIG_PILEUP)
        pr = np.zeros(ns, dtype=_READ_PLACE) if per_read else None
        par = _int_params(_lib.PileupParams, params, "pileup")
        st = _lib.PileupStats()
        check(self.ctx._L.mgta_reads_pileup(self.h, reads.h, int(bool(reads_reversed)), ns, buf, offsets.ctypes.data, n, C.byref(par) if params else None,
                                            counts.ctypes.data if total else None, uniq.ctypes.data if total else None, rec.ctypes.data if n else None,
                                            pr.ctypes.data if per_read and ns else None, C.byref(st)), "mgta_reads_pileup")
        return dict(counts=counts, uniq=uniq, contigs=rec, offsets=offsets.astype(np.int64), stats=st.as_dict(), reads=pr)

    def pileup_gapped(self, reads: "Reads", seqs, n_short_reads: int | None = None, params: dict | None = None, per_read: bool = False,
                      reads_reversed: bool = True, gap_cap: int | None = None) -> dict:
        """mgta_reads_pileup_gapped: Graph.pileup with reads placed across one insertion or deletion (the rule: include/megagta_hip.h).
        params = the three of pileup and max_gap=, gap_open=, gap_extend=, 0 or missing = the default of each.  -> the dict of
        Graph.pileup with reads = gapped.PLACE_DTYPE records and gaps = gapped.GAP_DTYPE records, sorted by the library.  The buffer
        of the gap records is sized from the reads scanned and the call repeated once with the count the library names."""
        buf, offsets, n = _pack(seqs)
        ns = reads.n_reads if n_short_reads is None else int(n_short_reads)
        total = int(offsets[-1])
        counts = np.zeros((total, 4), dtype=np.uint32)
        uniq = np.zeros(total, dtype=np.uint32)
        rec = np.zeros(n, dtype=_CONTIG_PILEUP)
        pr = np.zeros(ns, dtype=_GAP_PLACE) if per_read else None
        par = _int_params(_lib.GappedParams, params, "gapped pileup")
        st = _lib.GappedStats()
        cap = max(16, ns // 8) if gap_cap is None else int(gap_cap)
        for attempt in (0, 1):
            gaps = np.zeros(cap, dtype=_GAP_REC)
            rc = self.ctx._L.mgta_reads_pileup_gapped(self.h, reads.h, int(bool(reads_reversed)), ns, buf, offsets.ctypes.data, n,
                                                      C.byref(par) if params else None, counts.ctypes.data if total else None, uniq.ctypes.data if total else None,
                                                      rec.ctypes.data if n else None, pr.ctypes.data if per_read and ns else None, gaps.ctypes.data if cap else None,
                                                      cap, C.byref(st))
            if rc == -1 and attempt == 0 and gap_cap is None and st.n_gap_placements > cap:
                cap = int(st.n_gap_placements)
                continue
            check(rc, "mgta_reads_pileup_gapped")
            break
        return dict(counts=counts, uniq=uniq, contigs=rec, offsets=offsets.astype(np.int64), stats=st.as_dict(), reads=pr, gaps=gaps[:int(st.n_gap_placements)].copy())

    def denovo(self, max_tip_len: int = 150, no_bubble: bool = False, min_contig: int = 0) -> tuple[str, dict]:
        """`megagta denovo` (main_assemble, assembler.cpp:98-167): tips, bubbles, unitigs -> (text of PREFIX.contigs.fa, stats).
        The result is the reference's one-thread output.  CONSUMES the validity bits of this graph."""
        text, n, st = C.c_void_p(), C.c_uint64(), _lib.DenovoStats()
        check(self.ctx._L.mgta_denovo(self.h, max_tip_len, int(no_bubble), min_contig, C.byref(text), C.byref(n), C.byref(st)), "mgta_denovo")
        try:      # (ctypes.string_at takes a C int: a 100 M-read graph gives > 2^31 characters)
            fasta = bytes(memoryview((C.c_char * n.value).from_address(text.value))).decode() if n.value else ""
        finally:
            self.ctx._L.mgta_host_free(text)
        return fasta, st.as_dict()

    def free(self):
        if getattr(self, "h", None):
            self.ctx._L.mgta_sdbg_free(self.h)
            self.h = None

    __del__ = free


def link_pairs(pairs, n_residues, lens) -> dict:
    """mgta_pairs_link: the linkage of `Context.cluster` alone, on the host, no context and no device: pairs = the kept pairs of n rows
    ascending by (i, j) (a ROW_PAIR array, or tuples (i, j, n_diff, n_overlap)), n_residues = the residue columns of every row
    (0 = unaligned), lens -> dict(cluster, rep, rep_diff, rep_overlap, stats)."""
    p = _pair_array(pairs)
    nr, ln, n = _residues_and_lens(n_residues, lens)
    cl, rep, rd, ro = _linkage_outputs(max(1, n))
    st = _lib.ClusterStats()
    check(_lib.load().mgta_pairs_link(p.ctypes.data if p.size else None, p.size, nr.ctypes.data, ln.ctypes.data, n, cl.ctypes.data, rep.ctypes.data, rd.ctypes.data,
                                      ro.ctypes.data, C.byref(st)), "mgta_pairs_link")
    return _linkage_result(cl[:n], rep[:n], rd[:n], ro[:n], st)


def tree_cut(pairs, merges, n_residues, lens, cutoff: float) -> dict:
    """mgta_tree_cut: the clusters at `cutoff` read off the merge tree of `pairs` (Context.pairs_tree / Context.clusters), on the host,
    no context and no device: what link_pairs gives for the pairs kept at `cutoff` -> dict(cluster, rep, rep_diff, rep_overlap, stats);
    stats["n_cut_fallbacks"] = 1 when the kept rule split equal fractions and the host linkage ran instead."""
    p = _pair_array(pairs)
    m = np.ascontiguousarray(merges, dtype=TREE_MERGE) if isinstance(merges, np.ndarray) else np.array([tuple(x) for x in merges], dtype=TREE_MERGE)
    nr, ln, n = _residues_and_lens(n_residues, lens)
    cl, rep, rd, ro = _linkage_outputs(max(1, n))
    st = _lib.TreeStats()
    check(_lib.load().mgta_tree_cut(p.ctypes.data if p.size else None, p.size, m.ctypes.data if m.size else None, m.size, nr.ctypes.data, ln.ctypes.data, n,
                                    float(cutoff), cl.ctypes.data, rep.ctypes.data, rd.ctypes.data, ro.ctypes.data, C.byref(st)), "mgta_tree_cut")
    return _linkage_result(cl[:n], rep[:n], rd[:n], ro[:n], st)


class DeviceHmm:
    """Profile-HMM tables on the device (mgta_hmm) <-> ProfileHMM + MostProbablePath (profile_hmm.h, most_probable_path.h)."""

    def __init__(self, ctx: Context, hm):
        self.ctx, self.M, self.A = ctx, hm.M, hm.A
        msc = np.ascontiguousarray(hm.msc, dtype=np.float64)
        tsc = np.ascontiguousarray(hm.tsc, dtype=np.float64)
        mx = np.ascontiguousarray(hm.max_match, dtype=np.float64)
        h = np.ascontiguousarray(hm.h, dtype=np.float64)
        alpha = np.ascontiguousarray(hm.alpha, dtype=np.int32)
        out = C.c_void_p()
        check(ctx._L.mgta_hmm_load(ctx.h, hm.M, hm.A, msc.ctypes.data, tsc.ctypes.data, mx.ctypes.data, h.ctypes.data, alpha.ctypes.data,
                                   C.byref(out)), "mgta_hmm_load")
        self.h = out

    def free(self):
        if getattr(self, "h", None):
            self.ctx._L.mgta_hmm_free(self.h)
            self.h = None

    __del__ = free


@dataclass
class SeedResult:
    """One seed: HMMGraphSearch::search (hmm_graph_search.h:60-81)"""
    left: str          # already reverse-complemented
    right: str
    right_side: dict
    left_side: dict

    def contig(self, kmer: str) -> str:
        return self.left + kmer.lower() + self.right


def _set_cost(ctx: "Context", cost_rate) -> None:
    """cost_rate: an int (mgta_ctx_set_search_cost_rate) or (rate, knee, rate beyond the knee) (mgta_ctx_set_search_cost_curve)"""
    if isinstance(cost_rate, (tuple, list)):
        rate, knee, rate2 = (int(x) for x in cost_rate)
        if knee:
            check(ctx._L.mgta_ctx_set_search_cost_curve(ctx.h, rate, knee, rate2), "mgta_ctx_set_search_cost_curve")
            return
        cost_rate = rate
    check(ctx._L.mgta_ctx_set_search_cost_rate(ctx.h, int(cost_rate)), "mgta_ctx_set_search_cost_rate")


def _seeds(graph: "Graph", kmers: list[str], start_states, cost_rate, run: "Context | None" = None) -> tuple[bytes, np.ndarray, int]:
    """what both searches do first: the cost rate set (on the context the batch runs on: the graph's own unless `run` names another), then
    (the first k + 1 letters of every seed k-mer back to back, the start states as int32, the number of seeds)"""
    _set_cost(graph.ctx if run is None else run, cost_rate)
    klen = graph.k + 1
    if any(len(s) < klen for s in kmers):
        raise MegaGtaError(f"seed k-mer shorter than k+1={klen}")
    return "".join(s[:klen] for s in kmers).encode(), np.ascontiguousarray(start_states, dtype=np.int32), len(kmers)


def astar_search(graph: "Graph", fwd: DeviceHmm, rev: DeviceHmm, kmers: list[str], start_states, prune_len: int = 20,
                 low_cov_penalty: float = 0.5, cache_mode: int = 0, cost_rate=0, run: "Context | None" = None) -> tuple[list[SeedResult], dict]:
    """Batched HMM-guided A* (mgta_astar_batch).  start_states[i] = model position - 1 (search.cpp:157).
    cache_mode = B >= 1 shares paths between seeds: seed j's path (c_j expansions) is seen by the seeds >= j + B + c_j // cost_rate
    (cost_rate 0: no cost term; B = 1 then is the reference's sequential run; cost_rate < 0: j + B + c_j * |cost_rate|;
    cost_rate = (rate, knee, rate2): c_j // rate up to `knee` expansions, knee // rate + (c_j - knee) // rate2 beyond).
    cache_mode = -1: no ordering at all (timing-dependent, the reference's multi-thread behaviour).
    run = a context of the graph's device other than the graph's own: the batch takes that context's stream, work memory, cost rate and
    share of the CUs (mgta_astar_batch_on; Context.set_search_share), so that two threads can search one graph side by side."""
    buf, ss, n = _seeds(graph, kmers, start_states, cost_rate, run)
    results: list[SeedResult] = [None] * n

    def side(p):
        s = p.contents
        return dict(ok=s.ok, fval=s.fval, length=s.length, state_no=s.state_no, state=chr(s.state), partial=s.partial, node_id=s.node_id,
                    n_closed=s.n_closed, n_expanded=s.n_expanded, n_opened=s.n_opened, real_score=s.real_score, score=s.score)

    def sink(user, idx, left, ll, right, rl, rs, ls):
        results[idx] = SeedResult(left=C.string_at(left, ll).decode(), right=C.string_at(right, rl).decode(), right_side=side(rs),
                                  left_side=side(ls))
        return 0

    st = _lib.AstarStats()
    if run is not None:
        check(run._L.mgta_astar_batch_on(run.h, graph.h, fwd.h, rev.h, buf, ss.ctypes.data, n, prune_len, low_cov_penalty, cache_mode,
                                         _lib.CONTIG_SINK(sink), None, C.byref(st)), "mgta_astar_batch_on")
        return results, st.as_dict()
    check(graph.ctx._L.mgta_astar_batch(graph.h, fwd.h, rev.h, buf, ss.ctypes.data, n, prune_len, low_cov_penalty, cache_mode,
                                        _lib.CONTIG_SINK(sink), None, C.byref(st)), "mgta_astar_batch")
    return results, st.as_dict()


def astar_search_packed(graph: "Graph", fwd: DeviceHmm, rev: DeviceHmm, kmers: list[str], start_states, prune_len: int = 20,
                        low_cov_penalty: float = 0.5, cache_mode: int = 0, cost_rate=0, want_sides: bool = False):
    """astar_search with the results in flat arrays (mgta_astar_batch_packed): -> (contigs uint8[total], offsets int64[n + 1], stats[, sides]);
    contig i = contigs[offsets[i]:offsets[i + 1]] = left + lower-cased k-mer + right.  No Python work per seed."""
    ctx = graph.ctx
    buf, ss, n = _seeds(graph, kmers, start_states, cost_rate)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    sides = (_lib.AstarSide * (2 * n))() if want_sides else None
    text, st = C.c_void_p(), _lib.AstarStats()
    check(ctx._L.mgta_astar_batch_packed(graph.h, fwd.h, rev.h, buf, ss.ctypes.data, n, prune_len, low_cov_penalty, cache_mode, C.byref(text),
                                         offsets.ctypes.data, C.cast(sides, C.c_void_p) if want_sides else None, C.byref(st)), "mgta_astar_batch_packed")
    try:
        total = int(offsets[n])
        contigs = np.frombuffer((C.c_char * total).from_address(text.value), dtype=np.uint8).copy() if total else np.zeros(0, np.uint8)
    finally:
        ctx._L.mgta_host_free(text)
    out = (contigs, offsets.astype(np.int64), st.as_dict())
    return out + (sides,) if want_sides else out


def counting_text(hist: np.ndarray) -> str:
    """PREFIX.counting as s1_post_proc writes it: one line `i cumulative_count` for i = 1..65535 (cx1_read2sdbg_s1.cpp:923-930)"""
    acc = np.cumsum(hist[1:])
    return "".join(f"{i} {int(a)}\n" for i, a in zip(range(1, 65536), acc))


class Reads:
    def __init__(self, ctx: Context, handle, n_reads: int):
        self.ctx, self.h, self.n_reads = ctx, handle, n_reads

    def free(self):
        if getattr(self, "h", None):
            self.ctx._L.mgta_reads_free(self.h)
            self.h = None

    __del__ = free


# ------------------------------------------------------------------------------------------------
# .sdbg.N / .sdbg_info files
# ------------------------------------------------------------------------------------------------
def write_sdbg(prefix: str, s: EdgeStream, num_files: int = 1) -> None:
    """SdbgWriter layout (sdbg_multi_io.h:83-187): per record uint16, then uint16 full multiplicity if
    mult > 254, then words_per_tip uint32 if tip; text index with one line per bucket
    `bucket file byte_offset num_items num_tips num_large_mul` (file = -1 for an empty bucket).
    Buckets are dealt to `num_files` files as contiguous ranges of roughly equal record count."""
    n = s.records.size
    rec = s.records
    is_large = (rec >> 8) == 255
    is_tip = ((rec >> 5) & 1).astype(bool)
    sz = 2 + 2 * is_large.astype(np.int64) + 4 * s.words_per_tip * is_tip.astype(np.int64)
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(sz, out=off[1:])
    buf = np.zeros(int(off[-1]), dtype=np.uint8)
    pos = off[:-1]

    def put16(at, vals):
        v = vals.astype("<u2").view(np.uint8).reshape(-1, 2)
        buf[at] = v[:, 0]
        buf[at + 1] = v[:, 1]

    put16(pos, rec)
    if is_large.any():
        put16(pos[is_large] + 2, s.large)
    if is_tip.any():
        tp = pos[is_tip] + 2 + 2 * is_large[is_tip].astype(np.int64)
        tb = s.tips.astype("<u4").view(np.uint8).reshape(-1, 4 * s.words_per_tip)
        for j in range(4 * s.words_per_tip):
            buf[tp + j] = tb[:, j]
    bstart = np.zeros(NUM_BUCKETS + 1, dtype=np.int64)
    np.cumsum(s.bucket_items, out=bstart[1:])
    cuts = [0]
    for f in range(1, num_files):
        cuts.append(max(cuts[-1], int(np.searchsorted(bstart, n * f // num_files, side="left"))))
    cuts.append(NUM_BUCKETS)
    large_cum = np.concatenate([[0], np.cumsum(is_large)])
    tip_cum = np.concatenate([[0], np.cumsum(is_tip)])
    lines = [f"k {s.k}\n", f"words_per_tip_label {s.words_per_tip}\n", f"num_buckets {NUM_BUCKETS}\n", f"num_threads {num_files}\n",
             f"total_size {n}\n", f"num_tips {int(is_tip.sum())}\n", f"large_multi {int(is_large.sum())}\n"]
    file_of = np.zeros(NUM_BUCKETS, dtype=np.int64)
    for f in range(num_files):
        b0, b1 = cuts[f], cuts[f + 1]
        file_of[b0:b1] = f
        buf[off[bstart[b0]]:off[bstart[b1]]].tofile(f"{prefix}.sdbg.{f}")
    for b in range(NUM_BUCKETS):
        i0, i1 = bstart[b], bstart[b + 1]
        if i1 == i0:
            lines.append(f"{b} -1 0 0 0 0\n")
        else:
            f = file_of[b]
            lines.append(f"{b} {f} {off[i0] - off[bstart[cuts[f]]]} {i1 - i0} {tip_cum[i1] - tip_cum[i0]} "
                         f"{large_cum[i1] - large_cum[i0]}\n")
    with open(prefix + ".sdbg_info", "w") as fh:
        fh.writelines(lines)


def read_sdbg(prefix: str) -> EdgeStream:
    """SdbgReader (sdbg_multi_io.h:240-382): files -> logical stream in bucket order."""
    with open(prefix + ".sdbg_info") as fh:
        hdr = {}
        for key in ("k", "words_per_tip_label", "num_buckets", "num_threads", "total_size", "num_tips", "large_multi"):
            name, val = fh.readline().split()
            if name != key:
                raise ValueError(f"{prefix}.sdbg_info: expected '{key}', got '{name}'")
            hdr[key] = int(val)
        rows = np.loadtxt(fh, dtype=np.int64).reshape(-1, 6)
    if hdr["num_buckets"] != NUM_BUCKETS or rows.shape[0] != NUM_BUCKETS:
        raise ValueError("unexpected bucket count")
    wpt = hdr["words_per_tip_label"]
    files = [np.fromfile(f"{prefix}.sdbg.{t}", dtype=np.uint8) for t in range(hdr["num_threads"])]
    recs, large, tips = [], [], []
    for b in range(NUM_BUCKETS):
        _, tid, offb, items, ntips, nlarge = rows[b]
        if tid < 0 or items == 0:
            continue
        nbytes = items * 2 + nlarge * 2 + ntips * 4 * wpt
        chunk = files[tid][offb:offb + nbytes]
        if ntips == 0 and nlarge == 0:
            recs.append(chunk.view("<u2"))
            continue
        p, r, lg, tp = 0, [], [], []
        for _ in range(items):
            it = int(chunk[p]) | (int(chunk[p + 1]) << 8)
            p += 2
            r.append(it)
            if (it >> 8) == 255:
                lg.append(int(chunk[p]) | (int(chunk[p + 1]) << 8))
                p += 2
            if (it >> 5) & 1:
                tp.append(chunk[p:p + 4 * wpt].view("<u4").copy())
                p += 4 * wpt
        recs.append(np.array(r, dtype=np.uint16))
        large.append(np.array(lg, dtype=np.uint16))
        if tp:
            tips.append(np.concatenate(tp))
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    return EdgeStream(k=hdr["k"], words_per_tip=wpt, bucket_items=rows[:, 3].copy(), records=cat(recs, np.uint16),
                      large=cat(large, np.uint16), tips=cat(tips, np.uint32), bucket_large=rows[:, 5].copy(),
                      bucket_tips=rows[:, 4].copy())
