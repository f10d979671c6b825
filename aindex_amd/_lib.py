"""ctypes binding of libaindex_hip.so (the C ABI in include/aindex_hip.h).

The HIP library is the only compute path: if it cannot be loaded, importing this module raises —
there is no CPU fallback. torch (if importable) is imported first so that the process-wide HIP
runtime is the one PyTorch ships and device pointers of torch tensors are valid inside our kernels.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
LIB_PATH = os.path.join(_HERE, "lib", "libaindex_hip.so")
CSRC = os.path.join(_HERE, "csrc")
HEADER = os.path.join(ROOT, "include", "aindex_hip.h")

AIX_OK = 0
AIX_ERR_CONFLICT = -12
AIX_ERR_ARG = -1
AIX_ERR_FORMAT = -3
AIX_ERR_NOMEM = -4
AIX_ERR_HIP = -5
AIX_ERR_UNSUPPORTED = -6
AIX_ERR_MODE = -7
FMT_AUTO, FMT_PLAIN, FMT_FASTA, FMT_FASTQ = -1, 0, 1, 2
CANON_NONE, CANON_REF_X86, CANON_TRUE_RC = 0, 1, 2
TOTAL_13MERS = 4 ** 13
DIR_NEXT, DIR_PREV, DIR_BOTH = 0, 1, 2
WALK_GREEDY, WALK_UNITIG = 0, 1
STOP_NAMES = ("max_steps", "dead_end", "branch", "join", "loop")   # AIX_STOP_*
WALK_MAX_STEPS = 1 << 20
UNITIG_NONE = (1 << 64) - 1                                        # AIX_UNITIG_NONE
BUBBLE_NONE = 0xFFFFFFFF                                           # AIX_BUBBLE_NONE
GRAPH_MAX_THRESHOLD = 32767                                        # AIX_GRAPH_MAX_THRESHOLD
THREAD_NO_LINK = (1 << 64) - 1                                     # AIX_THREAD_NO_LINK
THREAD_BROKEN = (1 << 64) - 2                                      # AIX_THREAD_BROKEN
PHASE_NONE = 0xFF                                                  # AIX_PHASE_NONE
SPECTRUM_STATS = 8                                                 # AIX_SPECTRUM_STATS
STATS_FIELDS = ("n", "non_zero", "max", "min_non_zero", "sum", "non_zero_wide", "max_wide", "sum_wide")
FIX_NAMES = ("clean", "fixed", "partial", "unfixed", "short", "too_long", "bad_range")   # AIX_FIX_*
READFIX_MAX_LEN, READFIX_MAX_VERIFY, READFIX_MAX_FIXES = 4096, 16, 16
SEQFIND_TRIP_BYTES = 64                                            # AIX_SEQFIND_TRIP_BYTES of csrc/aix_seqhits.hpp: pattern bytes per verification trip
SEQEDIT_MAX_ED = 7                                                 # AIX_SEQEDIT_MAX_ED of csrc/aix_seqhits.hpp: the largest ed of aix_seq_edit
# aix_readfix_t: one 32-byte record per read
READFIX_FIELDS = [(f, "<u4") for f in ("status", "weak_before", "weak_after", "fixes", "n0", "nM", "trim_start", "trim_len")]


class AixError(RuntimeError):
    def __init__(self, status, what=""):
        self.status = status
        msg = lib().aix_strerror(status).decode() if _LIB is not None else str(status)
        super().__init__(f"{what}: {msg} (status {status})" if what else f"{msg} (status {status})")


class Info(C.Structure):
    _fields_ = [("k", C.c_uint32), ("device", C.c_uint32), ("n", C.c_uint64), ("mphf_n", C.c_uint64),
                ("hash_domain", C.c_uint64), ("seed", C.c_uint64), ("bitpairs", C.c_uint64),
                ("device_bytes", C.c_uint64), ("canonical_only", C.c_uint32), ("bucket_table", C.c_uint32),
                ("buckets", C.c_uint64), ("bucket_unfiled_keys", C.c_uint64), ("bucket_lanes", C.c_uint32), ("absence_filter_words", C.c_uint32),
                ("minimizer_lines", C.c_uint64), ("minimizer_unfiled_keys", C.c_uint64), ("count23_backend", C.c_uint32), ("count23_passes", C.c_uint32), ("positions_backend", C.c_uint32), ("reserved0", C.c_uint32),
                ("aindex_attached", C.c_uint32), ("ridx_on_device", C.c_uint32), ("aindex_entries", C.c_uint64), ("ridx_reads", C.c_uint64)]


class IngestStats(C.Structure):
    _fields_ = [("bytes_in", C.c_uint64), ("plain_bytes", C.c_uint64), ("parts", C.c_uint64), ("part_bytes", C.c_uint64), ("pieces", C.c_uint64),
                ("pinned_bytes", C.c_uint64), ("device_bytes", C.c_uint64), ("workspace_bytes", C.c_uint64), ("seconds_total", C.c_double), ("seconds_read", C.c_double),
                ("seconds_wait", C.c_double), ("seconds_h2d", C.c_double), ("seconds_normalise", C.c_double), ("seconds_compute", C.c_double), ("seconds_output", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# aix_cont_t: struct CONT of debrujin.hpp as one 32-byte record
CONT_FIELDS = [("tf", "<u4", (4,)), ("n", "<u4"), ("sum", "<u4"), ("best_tf", "<u4"), ("best_base", "<u4")]


def cont_dtype():
    """numpy dtype of one aix_cont_t record"""
    import numpy as np
    return np.dtype(CONT_FIELDS)


def readfix_dtype():
    """numpy dtype of one aix_readfix_t record"""
    import numpy as np
    return np.dtype(READFIX_FIELDS)


_LIB = None
vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int

# name -> (restype, argtypes); every symbol declared in include/aindex_hip.h
SIGNATURES = {
    "aix_version": (C.c_char_p, []),
    "aix_strerror": (C.c_char_p, [i32]),
    "aix_device_count": (i32, [C.POINTER(i32)]),
    "aix_pf_check": (i32, [vp, u64, C.POINTER(u64 * 4)]),
    "aix_index_open_23": (i32, [C.c_char_p, C.c_char_p, C.c_char_p, i32, C.POINTER(vp)]),
    "aix_index_open_13": (i32, [C.c_char_p, C.c_char_p, i32, C.POINTER(vp)]),
    "aix_index_create_23": (i32, [vp, u64, vp, vp, u64, i32, C.POINTER(vp)]),
    "aix_index_create_13": (i32, [vp, u64, vp, i32, C.POINTER(vp)]),
    "aix_index_close": (i32, [vp]),
    "aix_index_info": (i32, [vp, C.POINTER(Info)]),
    "aix_index_set_canonical_fastpath": (i32, [vp, i32]),
    "aix_index_set_fingerprint_filter": (i32, [vp, i32]),
    "aix_index_set_early_exit": (i32, [vp, i32]),
    "aix_index_set_bucket_table": (i32, [vp, i32, i32]),
    "aix_index_set_absence_filter": (i32, [vp, i32]),
    "aix_index_set_minimizer_table": (i32, [vp, i32]),
    "aix_index_set_tf_13": (i32, [vp, vp]),
    "aix_index_get_tf": (i32, [vp, vp, u64]),
    "aix_index_get_checker": (i32, [vp, vp, u64]),
    "aix_tf_batch_ascii": (i32, [vp, vp, u64, vp]),
    "aix_tf_batch_ascii_dev": (i32, [vp, vp, u64, vp, vp]),
    "aix_lookup_binned_stats": (i32, [vp, vp]),
    "aix_lookup_binned_coarse_stats": (i32, [vp, vp]),
    "aix_tf_batch_codes": (i32, [vp, vp, u64, vp]),
    "aix_tf_batch_codes_dev": (i32, [vp, vp, u64, vp, vp]),
    "aix_tf_batch_ragged": (i32, [vp, vp, vp, u64, vp]),
    "aix_tf_batch_ragged_dev": (i32, [vp, vp, vp, u64, vp, vp]),
    "aix_lines_batch_ascii_dev": (i32, [vp, vp, u64, vp, vp]),
    "aix_hash_batch_ascii": (i32, [vp, vp, u64, vp]),
    "aix_hash_batch_ascii_dev": (i32, [vp, vp, u64, vp, vp]),
    "aix_kid_strand_batch_ascii": (i32, [vp, vp, u64, vp, vp]),
    "aix_kid_strand_batch_ascii_dev": (i32, [vp, vp, u64, vp, vp, vp]),
    "aix_tf_both_batch_ascii": (i32, [vp, vp, u64, vp, vp]),
    "aix_tf_both_batch_ascii_dev": (i32, [vp, vp, u64, vp, vp, vp]),
    "aix_tf_total_batch_ascii": (i32, [vp, vp, u64, vp]),
    "aix_tf_total_batch_ascii_dev": (i32, [vp, vp, u64, vp, vp]),
    "aix_coverage_batch": (i32, [vp, vp, vp, u64, u32, vp, vp]),
    "aix_coverage_batch_dev": (i32, [vp, vp, vp, u64, u64, u32, vp, vp, vp]),
    "aix_count13": (i32, [vp, vp, u64, i32, vp]),
    "aix_count13_dev": (i32, [vp, vp, u64, vp, vp]),
    "aix_count23_fixed": (i32, [vp, vp, u64, i32, i32, vp]),
    "aix_count23_fixed_dev": (i32, [vp, vp, u64, i32, vp, vp]),
    "aix_ingest_warm": (i32, [i32]),
    "aix_count13_file": (i32, [vp, C.c_char_p, i32, C.c_char_p, vp, C.POINTER(IngestStats)]),
    "aix_count23_fixed_file": (i32, [vp, C.c_char_p, i32, i32, vp, C.POINTER(IngestStats)]),
    "aix_count_distinct_file": (i32, [C.c_char_p, i32, i32, i32, u64, i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64), C.POINTER(IngestStats)]),
    "aix_merge_runs_dev": (i32, [vp, vp, vp, u32, u64, i32, vp, C.POINTER(vp)]),
    "aix_count_distinct": (i32, [vp, u64, i32, i32, i32, u64, i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)]),
    "aix_positions_fill": (i32, [vp, vp, u64, vp, vp, u64, C.POINTER(u64)]),
    "aix_positions_total": (i32, [vp, C.POINTER(u64)]),
    "aix_positions_fill_dev": (i32, [vp, vp, u64, u64, vp, vp, u64, vp]),
    "aix_positions_bucket_counts": (i32, [vp, vp, u64, i32, vp]),
    "aix_aindex_attach": (i32, [vp, vp, vp, u64]),
    "aix_aindex_attach_dev": (i32, [vp, vp, vp, u64, vp]),
    "aix_aindex_detach": (i32, [vp]),
    "aix_ridx_sorted_disjoint": (i32, [vp, u64]),
    "aix_ridx_attach": (i32, [vp, vp, u64]),
    "aix_positions_query": (i32, [vp, vp, u64, u64, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]),
    "aix_positions_query_dev": (i32, [vp, vp, u64, u64, vp, vp, vp, vp, u64, C.POINTER(u64), vp]),
    "aix_positions_locate": (i32, [vp, vp, u64, vp, vp]),
    "aix_positions_locate_dev": (i32, [vp, vp, u64, vp, vp, vp]),
    "aix_reads_attach": (i32, [vp, vp, u64]),
    "aix_reads_attach_dev": (i32, [vp, vp, u64, vp]),
    "aix_reads_detach": (i32, [vp]),
    "aix_reads_info": (i32, [vp, C.POINTER(u64 * 2)]),
    "aix_reads_fetch": (i32, [vp, vp, vp, vp, u64, C.POINTER(vp), C.POINTER(vp)]),
    "aix_reads_fetch_dev": (i32, [vp, vp, vp, vp, u64, vp, vp, u64, C.POINTER(u64), vp]),
    "aix_reads_fetch_rid": (i32, [vp, vp, u64, C.POINTER(vp), C.POINTER(vp)]),
    "aix_reads_fetch_rid_dev": (i32, [vp, vp, u64, vp, vp, u64, C.POINTER(u64), vp]),
    "aix_reads_by_kmers": (i32, [vp, vp, u64, u64, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]),
    "aix_reads_by_kmers_dev": (i32, [vp, vp, u64, u64, vp, vp, vp, u64, vp, u64, C.POINTER(u64 * 2), vp]),
    "aix_neighbours": (i32, [vp, vp, vp, u64, i32, u32, vp]),
    "aix_neighbours_dev": (i32, [vp, vp, vp, u64, i32, u32, vp, vp]),
    "aix_walk": (i32, [vp, vp, vp, u64, i32, u64, u32, i32, vp, vp, vp, vp, vp]),
    "aix_walk_dev": (i32, [vp, vp, vp, u64, i32, u64, u32, i32, vp, vp, vp, vp, vp, vp]),
    "aix_unitigs_layout_dev": (i32, [vp, u32, vp, vp, vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), vp]),
    "aix_unitigs_emit_dev": (i32, [vp, u32, vp, vp, vp, u64, vp, vp, vp, vp, vp, vp, vp, vp]),
    "aix_unitigs": (i32, [vp, u32, C.POINTER(u64)] + [C.POINTER(vp)] * 10),
    "aix_unitig_links_dev": (i32, [vp, u32, vp, vp, vp, u64, vp, vp, vp, u64, C.POINTER(u64), vp]),
    "aix_unitig_bubbles_dev": (i32, [u64, vp, vp, u64, vp, vp]),
    "aix_unitig_links": (i32, [vp, u32, C.POINTER(u64), C.POINTER(u64)] + [C.POINTER(vp)] * 3),
    "aix_graph_mark_dev": (i32, [u64, vp, vp, vp, vp, vp, u64, vp, u32, u32, vp, C.POINTER(u64), C.POINTER(u64), vp]),
    "aix_graph_compact_layout_dev": (i32, [u64, vp, vp, vp, vp, vp, u64, vp, vp, vp, vp] + [C.POINTER(u64)] * 4 + [vp]),
    "aix_graph_compact_emit_dev": (i32, [u64] + [vp] * 8 + [u64] + [vp] * 4 + [u64] * 3 + [vp] * 9),
    "aix_graph_clean": (i32, [u64] + [vp] * 8 + [u64, u32, u32] + [C.POINTER(u64)] * 4 + [C.POINTER(vp)] * 12),
    "aix_graph_kidmap_dev": (i32, [u64, vp, vp, vp, u64] + [vp] * 8),
    "aix_thread_nodes_dev": (i32, [u64, vp, vp, vp, u64, vp, vp, vp]),
    "aix_seq_thread_dev": (i32, [vp, vp, vp, u64, vp, u64, vp, vp, vp, vp, u64] + [vp] * 8 + [u64, C.POINTER(u64), vp]),
    "aix_seq_thread": (i32, [vp, u32, vp, vp, u64] + [C.POINTER(vp)] * 8 + [C.POINTER(u64)] * 2),
    "aix_thread_pairs_dev": (i32, [u64, vp, vp, u64, u64, vp, vp, vp, vp, C.POINTER(u64), vp]),
    "aix_graph_resolve_mark_dev": (i32, [u64, vp, vp, vp, vp, u64, vp, vp, u64, u64, u64, vp, vp] + [C.POINTER(u64)] * 3 + [vp]),
    "aix_graph_resolve_layout_dev": (i32, [u64, vp, u64, vp, vp, vp] + [C.POINTER(u64)] * 3 + [vp]),
    "aix_graph_resolve_emit_dev": (i32, [u64] + [vp] * 8 + [u64] + [vp] * 4 + [u64] * 4 + [vp] * 10),
    "aix_graph_resolve": (i32, [u64] + [vp] * 8 + [u64, vp, vp, u64, u64, u64] + [C.POINTER(u64)] * 4 + [C.POINTER(vp)] * 11),
    "aix_mate_links_dev": (i32, [u64, vp, vp, u64, vp, vp, vp, vp, vp, u64, vp, vp, u32, u32, vp, vp, vp, vp, vp]),
    "aix_mate_bundle_dev": (i32, [u64, vp, vp, u64, vp, vp, vp, vp, u64, C.POINTER(u64), vp]),
    "aix_scaffold_mark_dev": (i32, [u64] + [vp] * 6 + [u64, u32, u64, u64, u64, vp, vp, vp, C.POINTER(u64), vp]),
    "aix_scaffold_layout_dev": (i32, [u64, vp, vp, vp, vp, u32, vp, vp, vp, vp] + [C.POINTER(u64)] * 3 + [vp]),
    "aix_scaffold_emit_dev": (i32, [u64, vp, vp, vp, vp, u32, vp, vp, vp, vp, u64, u64, vp, vp, vp, vp, vp, vp]),
    "aix_scaffold": (i32, [u64, vp, vp, vp, u64, vp, vp, u32, u64, u64, u64, u32] + [C.POINTER(u64)] * 4 + [C.POINTER(vp)] * 12),
    "aix_gap_close_dev": (i32, [u64, vp, vp, vp, u64, vp, vp, u32, u32, u32, vp, vp, vp, vp, vp, u64, C.POINTER(u64), vp, vp, vp]),
    "aix_scaffold_fill_layout_dev": (i32, [u64, vp, vp, vp, u64, vp, vp, u32, u64, vp, vp, vp, vp, vp, vp, u64] + [vp] * 6 + [C.POINTER(u64)] * 2 + [vp]),
    "aix_scaffold_fill_emit_dev": (i32, [u64, vp, vp, u32, u64, vp, u64, vp, vp, vp, vp, vp, u64, vp, vp]),
    "aix_scaffold_fill": (i32, [u64, vp, vp, vp, vp, u64, vp, vp, u64, vp, vp, u32, u32, u32, u32] + [C.POINTER(u64)] * 3 + [C.POINTER(vp)] * 14),
    "aix_pile_place_dev": (i32, [u64, vp, vp, u64, vp, vp, vp, vp, vp, u64, vp, u32, u32] + [vp] * 7 + [C.POINTER(u64)] * 2 + [vp]),
    "aix_pileup_dev": (i32, [vp, vp, u64, vp, u64, vp, vp, vp, vp, vp, u64, vp, vp, vp, vp, vp, vp]),
    "aix_pile_call_dev": (i32, [u64, vp, vp, vp, u32, u32, u32, u32, vp, C.POINTER(u64)] + [vp] * 7 + [u64, C.POINTER(u64), vp, vp, vp]),
    "aix_pileup": (i32, [vp, u32, vp, vp, u64, u32, u32] + [C.POINTER(u64)] * 3 + [C.POINTER(vp)] * 12),
    "aix_phase_observe_dev": (i32, [vp, vp, u64, u32, vp, u64, vp, vp, vp, vp, vp, u64, vp, u64, vp, vp, vp, vp, vp, vp, vp, u64, C.POINTER(u64), vp, vp, vp, u64,
                                    C.POINTER(u64), vp, vp]),
    "aix_phase_bundle_dev": (i32, [u64, u64, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(u64), vp]),
    "aix_phase_solve_dev": (i32, [u64, vp, vp, u64, vp, vp, vp, u32, u32, vp, vp, vp, vp, vp, vp]),
    "aix_phase_tag_dev": (i32, [u64, vp, u64, vp, vp, u64, vp, vp, vp, vp, vp, vp, vp]),
    "aix_phase_solve": (i32, [u64, vp, u64, vp, vp, vp, u32, u32, C.POINTER(u64)] + [C.POINTER(vp)] * 10),
    "aix_reads_fix": (i32, [vp, vp, u64, vp, vp, u64, u32, u32, u32, vp, vp, vp]),
    "aix_reads_fix_dev": (i32, [vp, vp, u64, vp, vp, u64, u32, u32, u32, vp, vp, vp, vp]),
    "aix_seq_hits": (i32, [vp, vp, vp, u64, u64, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]),
    "aix_seq_hits_dev": (i32, [vp, vp, vp, u64, u64, vp, vp, vp, vp, vp, vp, u64, C.POINTER(u64), vp]),
    "aix_seq_votes": (i32, [vp, vp, vp, u64, u64, u64, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]),
    "aix_seq_votes_dev": (i32, [vp, vp, vp, u64, u64, u64, vp, vp, vp, vp, vp, vp, vp, u64, C.POINTER(u64), vp]),
    "aix_seq_find": (i32, [vp, vp, vp, u64, u32, u64, u64, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]),
    "aix_seq_find_dev": (i32, [vp, vp, vp, u64, u32, u64, u64, vp, vp, vp, vp, vp, vp, u64, C.POINTER(u64), vp]),
    "aix_seq_edit": (i32, [vp, vp, vp, u64, u32, u64, u64, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                           C.POINTER(vp)]),
    "aix_seq_edit_dev": (i32, [vp, vp, vp, u64, u32, u64, u64, vp, vp, vp, vp, vp, vp, vp, u64, C.POINTER(u64), vp]),
    "aix_kmer_strands": (i32, [vp, vp, u64, u64, vp, vp, vp]),
    "aix_kmer_strands_dev": (i32, [vp, vp, u64, u64, vp, vp, vp, vp]),
    "aix_values_narrow_dev": (i32, [vp, u64, vp, vp]),
    "aix_spectrum_dev": (i32, [vp, i32, u64, u64, vp, vp, vp]),
    "aix_select_dev": (i32, [vp, u64, u32, u64, vp, vp, u64, C.POINTER(u64), C.POINTER(u64), vp]),
    "aix_kmer_values_dev": (i32, [vp, vp, vp]),
    "aix_tf_spectrum": (i32, [vp, u64, vp, vp]),
    "aix_tf_spectrum_dev": (i32, [vp, u64, vp, vp, vp]),
    "aix_top_kmers": (i32, [vp, u32, u64, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(u64), C.POINTER(u64)]),
    "aix_top_kmers_dev": (i32, [vp, u32, u64, vp, vp, vp, u64, C.POINTER(u64), C.POINTER(u64), vp]),
    "aix_kmers_by_kid": (i32, [vp, vp, u64, vp, vp, vp]),
    "aix_kmers_by_kid_dev": (i32, [vp, vp, u64, vp, vp, vp, vp]),
    "aix_positions_start": (i32, [vp, u64, C.POINTER(u64)]),
    "aix_positions_start_k": (i32, [vp, u64, i32, C.POINTER(u64)]),
    "aix_index_scatter_shard_codes_dev": (i32, [vp, u64, vp, vp, u64, u64, i32, vp, vp, vp, vp]),
    "aix_positions_indices_dev": (i32, [vp, vp, vp]),
    "aix_positions_bucket_counts_dev": (i32, [vp, vp, u64, u64, vp, vp]),
    "aix_positions_fill_shard_dev": (i32, [vp, vp, u64, u64, u64, vp, vp, vp, vp]),
    "aix_positions_fill_shard": (i32, [vp, vp, u64, i32, u64, vp, vp, u64]),
    "aix_window_codes_dev": (i32, [vp, u64, i32, i32, vp, vp]),
    "aix_normalize_reads": (i32, [vp, u64, i32, i32, vp, C.POINTER(u64)]),
    "aix_compute_reads": (i32, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p]),
    "aix_dat_load": (i32, [C.c_char_p, i32, C.POINTER(u64), C.POINTER(vp), C.POINTER(vp)]),
    "aix_pf_build_file": (i32, [C.c_char_p, C.POINTER(vp), C.POINTER(u64)]),
    "aix_kmers_write_text": (i32, [C.c_char_p, vp, vp, u64, i32]),
    "aix_file_write": (i32, [C.c_char_p, vp, u64]),
    "aix_ridx_load": (i32, [C.c_char_p, C.POINTER(u64), C.POINTER(vp)]),
    "aix_normalize_reads_dev": (i32, [vp, u64, i32, i32, vp, C.POINTER(u64), vp]),
    "aix_detect_format": (i32, [vp, u64]),
    "aix_synth_genome_dev": (i32, [u64, u64, vp, vp]),
    "aix_synth_kmers_dev": (i32, [u64, u64, u64, i32, vp, vp]),
    "aix_synth_mix23_dev": (i32, [u64, vp, u64, u64, u64, vp, vp]),
    "aix_synth_reads_dev": (i32, [u64, vp, u64, u64, u64, u32, i32, u32, vp, vp]),
    "aix_bench_gather_dev": (i32, [vp, u64, i32, i32, u64, u64, vp, vp]),
    "aix_pf_build": (i32, [vp, u64, u32, C.POINTER(vp), C.POINTER(u64)]),
    "aix_pf_build_ragged": (i32, [vp, vp, u64, C.POINTER(vp), C.POINTER(u64)]),
    "aix_pf_build_codes": (i32, [vp, u64, i32, C.POINTER(vp), C.POINTER(u64)]),
    "aix_index_scatter": (i32, [vp, u64, vp, vp, u64, i32, vp, vp]),
    "aix_count_distinct_dev": (i32, [vp, u64, i32, i32, u64, i32, vp, C.POINTER(vp)]),
    "aix_merge_counts_dev": (i32, [vp, vp, u64, u64, i32, vp, C.POINTER(vp)]),
    "aix_distinct_size": (i32, [vp, C.POINTER(u64)]),
    "aix_distinct_copy_dev": (i32, [vp, vp, vp, vp]),
    "aix_distinct_free": (None, [vp]),
    "aix_index_scatter_shard": (i32, [vp, u64, vp, vp, u64, u64, i32, vp, vp, vp]),
    "aix_index_build_23_codes_dev": (i32, [vp, u64, vp, vp, u64, i32, vp, C.POINTER(vp)]),
    "aix_pf_build_codes_dev": (i32, [vp, u64, i32, i32, vp, C.POINTER(vp), C.POINTER(u64)]),
    "aix_pf_build_all_13mers": (i32, [C.POINTER(vp), C.POINTER(u64)]),
    "aix_free": (None, [vp]),
    "aix_scratch_trim": (None, []),
    "aix_host_alloc": (i32, [u64, C.POINTER(vp)]),
    "aix_host_free": (i32, [vp]),
    "aix_debug_relocate_table": (i32, [vp, vp]),
    "aix_debug_relocate_bloom": (i32, [vp, u64]),
    "aix_selftest_lower_bound_dev": (i32, [vp, C.c_uint32, vp, C.c_uint32, vp, vp]),
    "aix_debug_rehome": (i32, [vp, C.c_uint32]),
    "aix_debug_pointers": (i32, [vp, C.POINTER(u64)]),
    "aix_debug_filter_words": (i32, [vp, vp, u64]),
    "aix_selftest_mod": (u64, [u64, u64]),
    "aix_selftest_revcomp": (u64, [u64, i32]),
}


def header_symbols():
    """Every function name declared in include/aindex_hip.h (used by the CPU export test)."""
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(aix_[a-z0-9_]+)\s*\(", text)))


def build(force: bool = False) -> str:
    """Compile libaindex_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp"))] + [HEADER]
    stale = (not os.path.exists(LIB_PATH)) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if force or stale:
        subprocess.check_call(["make", "-C", CSRC, "-j4"], stdout=subprocess.DEVNULL)
    return LIB_PATH


def lib():
    global _LIB
    if _LIB is None:
        if not os.environ.get("AIX_NO_TORCH"):                  # the command-line tools set it: they never touch a tensor, and importing torch costs seconds
            try:
                import torch  # noqa: F401  (loads PyTorch's HIP runtime first; see module docstring)
            except Exception:
                pass
        if not os.path.exists(LIB_PATH):
            build()
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)          # AttributeError here = ABI drift: fail loudly
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


def check(status: int, what: str = ""):
    if status != AIX_OK:
        raise AixError(status, what)


def device_count() -> int:
    n = i32(0)
    check(lib().aix_device_count(C.byref(n)), "aix_device_count")
    return n.value
