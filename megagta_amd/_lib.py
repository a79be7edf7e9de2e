"""ctypes loader of libmegagta_hip.so (the C ABI of include/megagta_hip.h).

There is no CPU fallback: if the HIP library is missing or no device is usable every call fails
loudly (MegaGtaError).

Note: PyTorch wheels bundle their own copy of the HIP runtime.  A process that uses both this library
and torch (bench.py, megagta_amd.dist) must `import torch` BEFORE the first call into this module so
that one runtime serves both; the library itself never needs torch.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MEGAGTA_HIP_LIB") or os.path.join(_HERE, "libmegagta_hip.so")   # (override: diagnostic builds)


class MegaGtaError(RuntimeError):
    pass


class Struct(C.Structure):
    """base of the mirrors: one class per `typedef struct mgta_*` of the header, listed in STRUCTS (tests/test_abi_layout_host.py has the C
    compiler check every one of them against the header)"""
    _not_shown = ()

    def as_dict(self) -> dict:
        """the members in order, an array member as a list"""
        d = {n: getattr(self, n) for n, _ in self._fields_ if n not in self._not_shown}
        return {n: list(v) if isinstance(v, C.Array) else v for n, v in d.items()}


class DenovoStats(Struct):
    _fields_ = [("n_tips", C.c_int64), ("n_bubbles", C.c_int64), ("n_bubble_candidates", C.c_int64), ("n_bubble_rounds", C.c_int64),
                ("n_paths", C.c_int64), ("n_unitig_sweeps", C.c_int64), ("n_contigs", C.c_int64), ("total_len", C.c_int64),
                ("ms_tips", C.c_float), ("ms_bubbles", C.c_float), ("ms_unitigs", C.c_float)]


class BuildStats(Struct):
    _fields_ = [("k", C.c_int32), ("words_per_key", C.c_int32), ("words_per_tip", C.c_int32), ("n_passes", C.c_int32),
                ("n_reads", C.c_int64), ("n_kmers", C.c_int64), ("n_items", C.c_int64), ("n_edges", C.c_int64),
                ("n_tips", C.c_int64), ("n_large", C.c_int64), ("n_sort_launches", C.c_int64), ("ms_total", C.c_double),
                ("ms_count", C.c_double), ("ms_gen", C.c_double), ("ms_sort", C.c_double), ("ms_emit", C.c_double),
                ("ms_d2h", C.c_double), ("ms_sort_scatter", C.c_double), ("ms_local_sort", C.c_double), ("n_big_segments", C.c_int64), ("n_lsd_tiles", C.c_int64),
                ("bytes_peak", C.c_uint64), ("ms_stage1", C.c_double), ("n_fused_passes", C.c_int64),
                ("n_wide_passes", C.c_int64), ("n_split_levels", C.c_int64)]


class AstarSide(Struct):
    _fields_ = [("ok", C.c_int32), ("fval", C.c_int32), ("length", C.c_int32), ("state_no", C.c_int32), ("state", C.c_int32),
                ("partial", C.c_int32), ("node_id", C.c_int64), ("n_closed", C.c_int64), ("n_expanded", C.c_int64),
                ("n_opened", C.c_int64), ("real_score", C.c_double), ("score", C.c_double)]


class AstarStats(Struct):
    _fields_ = [("n_seeds", C.c_int64), ("n_expansions", C.c_int64), ("n_opened", C.c_int64), ("n_retries", C.c_int64),
                ("ms_total", C.c_double), ("ms_kernel", C.c_double), ("n_grown", C.c_int64), ("n_rehash", C.c_int64),
                ("n_recycled", C.c_int64), ("pool_bytes", C.c_uint64), ("pool_used", C.c_uint64), ("n_resumes", C.c_int64),
                ("reserve_bytes", C.c_uint64), ("reserve_used", C.c_uint64), ("max_search_nodes", C.c_int64),
                ("max_search_expansions", C.c_int64), ("order_abandoned", C.c_int64), ("n_cache_drops", C.c_int64), ("hmm_in_lds", C.c_int64), ("n_over_limit", C.c_int64), ("ms_queue_drained", C.c_double)]


class LineProbe(Struct):
    _fields_ = [("waves_per_cu", C.c_int32), ("groups", C.c_int32), ("unroll", C.c_int32), ("dependent", C.c_int32), ("steps", C.c_uint64),
                ("lines_in_flight_per_cu", C.c_int32), ("pad_", C.c_int32), ("lines", C.c_uint64), ("ms", C.c_double), ("gb_per_s", C.c_double),
                ("ns_per_step", C.c_double)]
    _not_shown = ("pad_",)


class ContigCov(Struct):
    _fields_ = [("sum", C.c_uint64), ("len", C.c_uint32), ("n_windows", C.c_uint32), ("n_covered", C.c_uint32), ("min", C.c_uint32),
                ("max", C.c_uint32), ("median", C.c_uint32)]


class CoverageStats(Struct):
    _fields_ = [("n_contigs", C.c_int64), ("n_windows", C.c_int64), ("n_walked", C.c_int64), ("n_index_searches", C.c_int64),
                ("n_batches", C.c_int64), ("groups_per_cu", C.c_int64), ("ms_kernel", C.c_double), ("ms_walk", C.c_double)]


class ContigShare(Struct):
    _fields_ = [("mass", C.c_uint64), ("len", C.c_uint32), ("n_windows", C.c_uint32), ("n_covered", C.c_uint32), ("n_unique", C.c_uint32),
                ("max_share", C.c_uint32), ("reserved_", C.c_uint32)]


class ShareStats(Struct):
    _fields_ = [("n_contigs", C.c_int64), ("n_windows", C.c_int64), ("n_walked", C.c_int64), ("n_index_searches", C.c_int64), ("n_batches", C.c_int64),
                ("n_covered", C.c_int64), ("n_distinct_edges", C.c_int64), ("total_mult", C.c_uint64), ("total_mass", C.c_uint64),
                ("table_slots", C.c_uint64), ("table_bytes", C.c_uint64), ("window_bytes", C.c_uint64), ("ms_walk", C.c_double), ("ms_count", C.c_double),
                ("ms_share", C.c_double), ("ms_total", C.c_double)]


class MatchStats(Struct):
    _fields_ = [("n_contigs", C.c_int64), ("n_contig_windows", C.c_int64), ("n_marked_edges", C.c_int64), ("n_reads", C.c_int64),
                ("n_read_windows", C.c_int64), ("n_walked", C.c_int64), ("n_index_searches", C.c_int64), ("n_matched_reads", C.c_int64),
                ("groups_per_cu", C.c_int64), ("ms_mark", C.c_double), ("ms_walk", C.c_double)]


class SampleCovStats(Struct):
    _fields_ = [("n_contigs", C.c_int64), ("n_windows", C.c_int64), ("n_walked", C.c_int64), ("n_index_searches", C.c_int64), ("n_batches", C.c_int64),
                ("n_covered", C.c_int64), ("n_keys", C.c_int64), ("n_libs", C.c_int64), ("n_reads", C.c_int64), ("n_read_windows", C.c_int64),
                ("n_read_walked", C.c_int64), ("n_read_index_searches", C.c_int64), ("n_hit_windows", C.c_int64), ("groups_per_cu", C.c_int64),
                ("total_mass", C.c_uint64), ("table_slots", C.c_uint64), ("table_bytes", C.c_uint64), ("window_bytes", C.c_uint64),
                ("count_bytes", C.c_uint64), ("ms_mark", C.c_double), ("ms_scan", C.c_double), ("ms_mass", C.c_double), ("ms_total", C.c_double)]


class DerepStats(Struct):
    _fields_ = [("n_seqs", C.c_int64), ("n_letters", C.c_int64), ("n_first", C.c_int64), ("n_duplicates", C.c_int64), ("n_contained", C.c_int64),
                ("n_kept", C.c_int64), ("n_windows", C.c_int64), ("anchor_len", C.c_int64), ("n_compares", C.c_int64), ("ms_dups", C.c_double),
                ("ms_table", C.c_double), ("ms_verify", C.c_double)]


class AlignRec(Struct):
    _fields_ = [("score", C.c_double), ("status", C.c_int32), ("model_from", C.c_int32), ("model_to", C.c_int32), ("n_match", C.c_int32),
                ("n_insert", C.c_int32), ("n_delete", C.c_int32)]


class AlignStats(Struct):
    _fields_ = [("n_seqs", C.c_int64), ("n_aligned", C.c_int64), ("n_unaligned", C.c_int64), ("n_cells", C.c_int64), ("n_batches", C.c_int64),
                ("blocks_per_cu", C.c_int64), ("waves_per_block", C.c_int64), ("grid_blocks", C.c_int64), ("lds_bytes", C.c_int64),
                ("msc_in_lds", C.c_int64), ("ms_fill", C.c_double), ("ms_trace", C.c_double)]


class PostRec(Struct):
    _fields_ = [("fwd", C.c_double), ("bwd", C.c_double), ("status", C.c_int32), ("pad", C.c_int32)]


class PostStats(Struct):
    _fields_ = [("n_seqs", C.c_int64), ("n_scored", C.c_int64), ("n_unaligned", C.c_int64), ("n_cells", C.c_int64), ("n_batches", C.c_int64),
                ("workgroups", C.c_int64), ("waves_per_block", C.c_int64), ("blocks_per_cu", C.c_int64), ("lds_bytes", C.c_int64),
                ("msc_in_lds", C.c_int64), ("peak_bytes", C.c_int64), ("ms_forward", C.c_double), ("ms_backward", C.c_double)]


class RowPair(Struct):
    _fields_ = [("i", C.c_int32), ("j", C.c_int32), ("n_diff", C.c_uint16), ("n_overlap", C.c_uint16)]


class TreeMerge(Struct):
    _fields_ = [("a", C.c_int32), ("b", C.c_int32), ("n_diff", C.c_uint16), ("n_overlap", C.c_uint16)]


class ClusterStats(Struct):
    _fields_ = [("n_rows", C.c_int64), ("n_unaligned", C.c_int64), ("n_pairs_kept", C.c_int64), ("n_clusters", C.c_int64), ("n_singletons", C.c_int64),
                ("largest_cluster", C.c_int64), ("n_components", C.c_int64), ("n_tiles", C.c_int64), ("n_link_pops", C.c_int64),
                ("blocks_per_cu", C.c_int64), ("grid_blocks", C.c_int64), ("lds_bytes", C.c_int64), ("peak_bytes", C.c_int64),
                ("ms_pairs", C.c_double), ("ms_link", C.c_double)]


class TreeStats(Struct):
    _fields_ = [("n_rows", C.c_int64), ("n_pairs", C.c_int64), ("n_merges", C.c_int64), ("n_rounds", C.c_int64), ("n_entries_visited", C.c_int64),
                ("n_lists_rewritten", C.c_int64), ("n_cut_fallbacks", C.c_int64), ("n_unaligned", C.c_int64), ("n_clusters", C.c_int64),
                ("n_singletons", C.c_int64), ("largest_cluster", C.c_int64), ("peak_bytes", C.c_int64), ("ms_pairs", C.c_double), ("ms_build", C.c_double),
                ("ms_rounds", C.c_double), ("ms_cut", C.c_double)]


class NearestRec(Struct):
    _fields_ = [("status", C.c_int32), ("ref", C.c_int32), ("score", C.c_int32), ("ref_from", C.c_int32), ("ref_to", C.c_int32), ("n_match", C.c_int32),
                ("n_ident", C.c_int32), ("n_insert", C.c_int32), ("n_delete", C.c_int32)]


class NearestStats(Struct):
    _fields_ = [("n_seqs", C.c_int64), ("n_refs", C.c_int64), ("n_pairs", C.c_int64), ("n_unaligned", C.c_int64), ("n_cells", C.c_int64),
                ("n_trace_cells", C.c_int64), ("n_batches", C.c_int64), ("n_segments", C.c_int64), ("blocks_per_cu", C.c_int64),
                ("waves_per_block", C.c_int64), ("grid_blocks", C.c_int64), ("lds_bytes", C.c_int64), ("peak_bytes", C.c_int64),
                ("ms_score", C.c_double), ("ms_trace", C.c_double)]


class FrameshiftRec(Struct):
    _fields_ = NearestRec._fields_ + [("n_short", C.c_int32), ("n_long", C.c_int32)]


class FrameshiftStats(Struct):
    _fields_ = NearestStats._fields_ + [("n_shifted", C.c_int64)]


class ChimeraRec(Struct):
    _fields_ = [("status", C.c_int32), ("ref", C.c_int32), ("score", C.c_int32), ("brk", C.c_int32), ("left_ref", C.c_int32), ("left_score", C.c_int32),
                ("right_ref", C.c_int32), ("right_score", C.c_int32), ("two", C.c_int32), ("one", C.c_int32), ("gain", C.c_int32)]


class ChimeraStats(Struct):
    _fields_ = [("n_seqs", C.c_int64), ("n_refs", C.c_int64), ("n_clean", C.c_int64), ("n_chimeric", C.c_int64), ("n_unchecked", C.c_int64),
                ("n_cells", C.c_int64), ("n_parent_cells", C.c_int64), ("n_items", C.c_int64), ("n_parent_items", C.c_int64), ("n_segments", C.c_int64),
                ("n_groups", C.c_int64), ("grid_blocks", C.c_int64), ("waves_per_block", C.c_int64), ("blocks_per_cu", C.c_int64), ("lds_bytes", C.c_int64),
                ("bound_bytes", C.c_int64), ("peak_bytes", C.c_int64), ("ms_top", C.c_double), ("ms_parents", C.c_double)]


class PileupParams(Struct):
    _fields_ = [("min_anchors", C.c_int32), ("min_overlap", C.c_int32), ("max_mismatch_permille", C.c_int32)]


class ContigPileup(Struct):
    _fields_ = [("len", C.c_uint32), ("n_covered", C.c_uint32), ("min_depth", C.c_uint32), ("max_depth", C.c_uint32), ("n_placed", C.c_uint64),
                ("n_unique", C.c_uint64), ("depth_sum", C.c_uint64), ("mismatch_sum", C.c_uint64)]


class ReadPlace(Struct):
    _fields_ = [("score", C.c_int32), ("contig", C.c_int32), ("diag", C.c_int32), ("orient", C.c_int32), ("n_placed", C.c_uint32), ("n_mismatch", C.c_uint32)]


class PileupStats(Struct):
    _fields_ = [("n_contigs", C.c_int64), ("n_contig_letters", C.c_int64), ("n_contig_windows", C.c_int64), ("n_keys", C.c_int64), ("n_occurrences", C.c_int64),
                ("n_reads", C.c_int64), ("n_read_windows", C.c_int64), ("n_hit_windows", C.c_int64), ("n_read_walked", C.c_int64),
                ("n_read_index_searches", C.c_int64), ("n_reads_with_candidate", C.c_int64), ("n_candidates", C.c_int64), ("n_verified", C.c_int64),
                ("n_reads_placed", C.c_int64), ("n_reads_multi", C.c_int64), ("n_placements", C.c_int64), ("n_bases_piled", C.c_int64),
                ("groups_per_cu", C.c_int64), ("peak_bytes", C.c_uint64), ("ms_keys", C.c_double), ("ms_index", C.c_double), ("ms_scan", C.c_double),
                ("ms_records", C.c_double), ("ms_total", C.c_double)]


class GappedParams(Struct):
    _fields_ = [("min_anchors", C.c_int32), ("min_overlap", C.c_int32), ("max_mismatch_permille", C.c_int32), ("max_gap", C.c_int32), ("gap_open", C.c_int32),
                ("gap_extend", C.c_int32)]


class GapPlace(Struct):
    _fields_ = ReadPlace._fields_ + [("diag2", C.c_int32), ("brk", C.c_uint32)]


class GapRec(Struct):
    _fields_ = [("read", C.c_uint64), ("contig", C.c_int32), ("pos", C.c_uint32), ("len", C.c_int32), ("brk", C.c_uint32), ("orient", C.c_int32),
                ("unique", C.c_int32)]


class GappedStats(Struct):
    _fields_ = PileupStats._fields_ + [("n_gap_candidates", C.c_int64), ("n_gap_passing", C.c_int64), ("n_reads_gapped", C.c_int64), ("n_gap_placements", C.c_int64),
                                       ("n_inserted", C.c_int64), ("n_deleted", C.c_int64), ("diag_list_entries", C.c_int64)]


class PhaseParams(Struct):
    _fields_ = [("max_span", C.c_int32)]


class PhaseStats(Struct):
    _fields_ = [("n_reads", C.c_int64), ("n_usable", C.c_int64), ("n_fragments", C.c_int64), ("n_mate_fragments", C.c_int64),
                ("n_fragments_allele", C.c_int64), ("n_fragments_linked", C.c_int64), ("n_alleles", C.c_int64), ("n_conflicts", C.c_int64),
                ("n_pair_adds", C.c_int64), ("n_sites", C.c_int64), ("n_pairs", C.c_int64), ("peak_bytes", C.c_uint64), ("ms_upload", C.c_double),
                ("ms_scan", C.c_double), ("ms_total", C.c_double)]


class RecruitParams(Struct):
    _fields_ = [("min_aa", C.c_int32), ("mode", C.c_int32), ("min_score", C.c_double)]


class RecruitRec(Struct):
    _fields_ = [("score", C.c_double), ("model_from", C.c_int32), ("model_to", C.c_int32), ("aa_from", C.c_uint16), ("aa_len", C.c_uint16),
                ("frame", C.c_uint8), ("status", C.c_uint8), ("pad", C.c_uint8 * 2)]


class RecruitStats(Struct):
    _fields_ = [("n_reads", C.c_int64), ("n_frames_scored", C.c_int64), ("n_cells", C.c_int64), ("n_unaligned", C.c_int64), ("n_unscored", C.c_int64),
                ("n_recruited", C.c_int64), ("n_recruited_frame", C.c_int64 * 6), ("blocks_per_cu", C.c_int64), ("waves_per_block", C.c_int64),
                ("grid_blocks", C.c_int64), ("lds_bytes", C.c_int64), ("msc_in_lds", C.c_int64), ("rows_per_wave", C.c_int64), ("chunk", C.c_int64),
                ("ms_scan", C.c_double), ("ms_fill", C.c_double)]


class SeedHit(Struct):
    _fields_ = [("read", C.c_uint64), ("pos_strand", C.c_uint32), ("ref", C.c_int32)]


# header name -> mirror, for every struct of include/megagta_hip.h
STRUCTS = {
    "mgta_build_stats": BuildStats, "mgta_contig_cov": ContigCov, "mgta_coverage_stats": CoverageStats, "mgta_contig_share": ContigShare,
    "mgta_share_stats": ShareStats, "mgta_match_stats": MatchStats, "mgta_sample_cov_stats": SampleCovStats, "mgta_pileup_params": PileupParams,
    "mgta_contig_pileup": ContigPileup, "mgta_read_place": ReadPlace, "mgta_pileup_stats": PileupStats, "mgta_gapped_params": GappedParams,
    "mgta_gap_place": GapPlace, "mgta_gap_rec": GapRec, "mgta_gapped_stats": GappedStats, "mgta_phase_params": PhaseParams, "mgta_phase_stats": PhaseStats,
    "mgta_recruit_params": RecruitParams, "mgta_recruit_rec": RecruitRec, "mgta_recruit_stats": RecruitStats, "mgta_derep_stats": DerepStats,
    "mgta_align_rec": AlignRec, "mgta_align_stats": AlignStats, "mgta_post_rec": PostRec, "mgta_post_stats": PostStats, "mgta_row_pair": RowPair,
    "mgta_cluster_stats": ClusterStats, "mgta_tree_merge": TreeMerge, "mgta_tree_stats": TreeStats, "mgta_nearest_rec": NearestRec,
    "mgta_nearest_stats": NearestStats, "mgta_frameshift_rec": FrameshiftRec, "mgta_frameshift_stats": FrameshiftStats, "mgta_chimera_rec": ChimeraRec,
    "mgta_chimera_stats": ChimeraStats, "mgta_seed_hit": SeedHit, "mgta_denovo_stats": DenovoStats, "mgta_astar_side": AstarSide,
    "mgta_astar_stats": AstarStats, "mgta_line_probe": LineProbe,
}

# the numpy record dtype of every struct that travels in arrays, derived from its mirror once: api.py and the stage modules give these
# objects their names (api.ALIGN_REC and align.REC are RECORDS[AlignRec], ...)
RECORDS = {c: np.dtype(c) for c in (ContigCov, ContigShare, ContigPileup, ReadPlace, GapPlace, GapRec, RecruitRec, AlignRec, PostRec, RowPair, TreeMerge,
                                    NearestRec, FrameshiftRec, ChimeraRec, SeedHit)}

EDGE_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_uint16), C.c_int64,
                        C.POINTER(C.c_uint16), C.c_int64, C.POINTER(C.c_uint32), C.c_int64)
CONTIG_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                          C.POINTER(AstarSide), C.POINTER(AstarSide))

# every symbol include/megagta_hip.h declares (tests/test_abi_and_host.py checks that the table names them all and the library exports them)
SYMBOLS = {
    "mgta_last_error": (C.c_char_p, []),
    "mgta_version": (C.c_char_p, []),
    "mgta_ctx_create": (C.c_void_p, [C.c_int]),
    "mgta_ctx_destroy": (None, [C.c_void_p]),
    "mgta_ctx_set_mem_limit": (C.c_int, [C.c_void_p, C.c_uint64]),
    "mgta_ctx_set_full_lsd": (C.c_int, [C.c_void_p, C.c_int]),
    "mgta_sort_plan": (C.c_int, [C.c_uint64, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mgta_sort_plan_wide": (C.c_int, [C.c_uint64, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mgta_reads_upload": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    "mgta_reads_adopt_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    "mgta_reads_free": (None, [C.c_void_p]),
    "mgta_sdbg_build_resident": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int32, C.c_int32,
                                          EDGE_SINK, C.c_void_p, C.POINTER(BuildStats)]),
    "mgta_sdbg_last_counting": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mgta_sdbg_last_emit_fused": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "mgta_sdbg_export_records_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "mgta_sdbg_build": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int,
                                 C.c_int, EDGE_SINK, C.c_void_p, C.POINTER(BuildStats)]),
    "mgta_findstart": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "mgta_sdbg_load_resident": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mgta_sdbg_load_files": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p]),
    "mgta_sdbg_invalid_bits": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mgta_ctx_set_search_cost_rate": (C.c_int, [C.c_void_p, C.c_int]),
    "mgta_ctx_set_search_cost_curve": (C.c_int, [C.c_void_p, C.c_int, C.c_uint64, C.c_int]),
    "mgta_ctx_set_search_arena": (C.c_int, [C.c_void_p, C.c_int, C.c_uint64]),
    "mgta_ctx_set_search_page_limit": (C.c_int, [C.c_void_p, C.c_int]),
    "mgta_ctx_device_memory": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "mgta_ctx_keep_stream": (C.c_int, [C.c_void_p, C.c_int]),
    "mgta_sdbg_stream_detach": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "mgta_stream_sizes": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "mgta_stream_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mgta_stream_free": (None, [C.c_void_p]),
    "mgta_sdbg_k": (C.c_int, [C.c_void_p]),
    "mgta_ctx_set_search_share": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "mgta_astar_batch_on": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_int, C.c_double,
                                     C.c_int, CONTIG_SINK, C.c_void_p, C.POINTER(AstarStats)]),
    "mgta_astar_batch_packed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_int, C.c_double, C.c_int,
                                         C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.POINTER(AstarStats)]),
    "mgta_reads_pack_text": (C.c_int, [C.c_void_p, C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "mgta_ctx_release_scratch": (C.c_int, [C.c_void_p]),
    "mgta_denovo": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mgta_host_free": (None, [C.c_void_p]),
    "mgta_sdbg_load": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int,
                                C.POINTER(C.c_void_p)]),
    "mgta_ctx_keep_multiplicity": (C.c_int, [C.c_void_p, C.c_int]),
    "mgta_ctx_set_coverage_batch": (C.c_int, [C.c_void_p, C.c_uint64]),
    "mgta_sdbg_load_large": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64,
                                      C.POINTER(C.c_void_p)]),
    "mgta_sdbg_edge_multiplicity": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "mgta_contig_coverage": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mgta_contig_share_coverage": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mgta_ctx_set_share_hash_bits": (C.c_int, [C.c_void_p, C.c_int]),
    "mgta_reads_match_contigs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_char_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "mgta_contig_sample_coverage": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_char_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mgta_reads_pileup": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_char_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "mgta_ctx_set_pileup_chunk": (C.c_int, [C.c_void_p, C.c_uint32]),
    "mgta_reads_pileup_gapped": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_char_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "mgta_phase_pairs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
    "mgta_reads_phase": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "mgta_ctx_set_phase_chunk": (C.c_int, [C.c_void_p, C.c_uint32]),
    "mgta_reads_recruit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mgta_ctx_set_recruit_chunk": (C.c_int, [C.c_void_p, C.c_uint32]),
    "mgta_seqs_derep": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mgta_ctx_set_derep_hash_bits": (C.c_int, [C.c_void_p, C.c_int]),
    "mgta_seqs_align": (C.c_int, [C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mgta_ctx_set_align_batch": (C.c_int, [C.c_void_p, C.c_int64]),
    "mgta_seqs_posterior": (C.c_int, [C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "mgta_ctx_set_posterior_batch": (C.c_int, [C.c_void_p, C.c_int64]),
    "mgta_rows_pairs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_double, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "mgta_rows_cluster": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    "mgta_pairs_link": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mgta_ctx_set_cluster_tile": (C.c_int, [C.c_void_p, C.c_int64]),
    "mgta_pairs_tree": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "mgta_tree_cut": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p]),
    "mgta_rows_clusters": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mgta_seqs_nearest": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_char_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mgta_ctx_set_nearest_batch": (C.c_int, [C.c_void_p, C.c_int64]),
    "mgta_seqs_frameshift": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_char_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32,
                                       C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mgta_seqs_chimera": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_char_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32,
                                    C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mgta_ctx_set_chimera_segment": (C.c_int, [C.c_void_p, C.c_int64]),
    "mgta_ctx_set_chimera_groups": (C.c_int, [C.c_void_p, C.c_int64]),
    "mgta_sdbg_free": (None, [C.c_void_p]),
    "mgta_sdbg_size": (C.c_int64, [C.c_void_p]),
    "mgta_sdbg_outgoing": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "mgta_sdbg_navigate": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "mgta_sdbg_index_edges": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "mgta_hmm_load": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.POINTER(C.c_void_p)]),
    "mgta_hmm_free": (None, [C.c_void_p]),
    "mgta_probe_random_lines": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(LineProbe), C.c_int]),
    "mgta_astar_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_int, C.c_double,
                                  C.c_int, CONTIG_SINK, C.c_void_p, C.POINTER(AstarStats)]),
}

_LIB = None


def load():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise MegaGtaError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(make -C megagta_amd/csrc). There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    _LIB = L
    return L


def check(rc: int, what: str):
    if rc != 0:
        raise MegaGtaError(f"{what} failed ({rc}): {load().mgta_last_error().decode()}")
