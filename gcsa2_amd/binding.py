"""ctypes binding of the C ABI (include/gcsa2_hip.h) + a host-side mirror of the reference's
query interface.

`GCSA` / `LCPArray` keep the reference's method names and argument meaning
(`include/gcsa/gcsa.h:96-210`, `include/gcsa/lcp.h:137-178`) so that parity tests read like the
reference's own checks; every method runs on the GPU through `libgcsa2_hip.so`.  There is no CPU
fallback: if the library or a device is missing, construction raises.
"""
import ctypes as C
import os
import sys
import numpy as np

from .hostview import (HostView, STNode, STNODE_DTYPE, UNKNOWN, make_host_view, concat_patterns,
                       u64p, u8p)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GCSA2_HIP_LIB") or os.path.join(_HERE, "lib", "libgcsa2_hip.so")   # override: A/B runs of two builds

STATUS_BUFFER_TOO_SMALL = -6
KMER_COUNTS = 1     # GCSA2_KMER_COUNTS
SUPPORT_PER_BIN = 1     # GCSA2_SUPPORT_PER_BIN
SUPPORT_STATS = ("windows", "found", "counted", "distinct", "values", "added", "dropped")     # gcsa2_support_stats
SPECTRUM_COUNTS = 1     # GCSA2_SPECTRUM_COUNTS
SPECTRUM_STATS = ("kmers", "nodes", "occurrences", "unique", "max_value")     # gcsa2_spectrum_stats
INDEX_KMER = ("sp", "ep", "count", "nodes", "k", "kmer0", "kmer1", "kmer2")     # gcsa2_index_kmer, the columns of list_kmers
CLASS_NONE = 0xFFFFFFFF     # GCSA2_CLASS_NONE
CLASS_LIMIT = 4096          # GCSA2_CLASS_LIMIT
CLASS_PER_WINDOW = 1        # GCSA2_CLASS_PER_WINDOW
CLASS_UNAMBIGUOUS = 2       # GCSA2_CLASS_UNAMBIGUOUS
CLASS_CALL = ("best", "best_votes", "second", "second_votes", "total", "counted")     # gcsa2_class_call
CLASS_STATS = ("windows", "found", "counted", "distinct", "values", "votes", "unclassified", "ambiguous")     # gcsa2_class_stats
TOP_LIMIT = 64              # GCSA2_TOP_LIMIT
TOP_SLOTS_DEFAULT = 512     # the default of GCSA2_TOP_SLOTS (the test knob of the top-classes calls)
CLASS_VOTE = np.dtype([("class_id", np.uint64), ("votes", np.uint64)])     # gcsa2_class_vote
TOP_SUMMARY = np.dtype([("voted", np.uint64), ("total", np.uint64), ("counted", np.uint64)])     # gcsa2_top_summary
CLUSTER_TOP_LIMIT = 64      # GCSA2_CLUSTER_TOP_LIMIT
CLUSTER_LDS_DEFAULT = 4096  # the default of GCSA2_CLUSTER_LDS (the test knob of the cluster calls)
CLUSTER = ("diag_min", "diag_max", "anchors", "starts", "covered", "read_begin", "read_end", "ref_begin")     # gcsa2_cluster
CLUSTER_SUMMARY = ("anchors", "unplaced", "clusters")     # gcsa2_cluster_summary
CLUSTER_STATS = ("groups", "invalid_groups", "seeds", "anchors", "unplaced", "clusters", "spilled")     # gcsa2_cluster_stats
from .binding_chains import (CHAIN_TOP_LIMIT, CHAIN_LOOKBACK_LIMIT, CHAIN_LDS_DEFAULT, CHAIN, CHAIN_ANCHOR, CHAIN_SUMMARY, CHAIN_STATS,
                             CHAIN_DEFAULTS, CHAIN_EXPORTS, ChainParams, ChainCalls, chain_params, declare_chain_calls)     # include/gcsa2_hip_chains.h
from .binding_strands import (STRAND_FORWARD, STRAND_REVERSE, STRAND_BOTH, CANONICAL_MINIMIZER, STRAND_EXPORTS, StrandCalls,
                              declare_strand_calls)     # include/gcsa2_hip_strands.h
from .binding_pairs import (PAIR_TOP_LIMIT, PAIR_FR, PAIR_RF, PAIR_FF, CHAIN_PAIR, PAIR_SUMMARY, PAIR_STATS, PAIR_DEFAULTS, PAIR_EXPORTS, PairParams,
                            PairCalls, pair_params, declare_pair_calls)     # include/gcsa2_hip_pairs.h
STATUS = {0: "OK", -1: "INVALID_ARGUMENT", -2: "NO_DEVICE", -3: "OUT_OF_MEMORY", -4: "HIP",
          -5: "MISSING_COMPONENT", -6: "BUFFER_TOO_SMALL"}

EXPORTS = [
    "gcsa2_device_count", "gcsa2_index_create", "gcsa2_index_destroy", "gcsa2_index_set_tables", "gcsa2_index_trim", "gcsa2_index_set_pipeline", "gcsa2_last_error",
    "gcsa2_size", "gcsa2_edge_count", "gcsa2_order", "gcsa2_sample_count", "gcsa2_sample_bits",
    "gcsa2_device", "gcsa2_device_bytes", "gcsa2_block_bits",
    "gcsa2_find_batch", "gcsa2_find_batch_packed", "gcsa2_find_packed_device", "gcsa2_find_device", "gcsa2_find_stats_device", "gcsa2_find_device_variant",
    "gcsa2_find_block_bytes", "gcsa2_kmer_table_k", "gcsa2_locate_table_bytes", "gcsa2_jump_table_bytes", "gcsa2_jump_mid", "gcsa2_jump_mid_default", "gcsa2_jump_branch", "gcsa2_jump_branch_default", "gcsa2_pair_block_bytes", "gcsa2_lf_batch", "gcsa2_lf_device",
    "gcsa2_lf_node_batch", "gcsa2_char_range", "gcsa2_lf_all_batch",
    "gcsa2_count_batch", "gcsa2_count_device",
    "gcsa2_locate_run", "gcsa2_locate_fetch", "gcsa2_locate_discard", "gcsa2_locate_device", "gcsa2_locate_into",
    "gcsa2_parent_batch", "gcsa2_parent_device", "gcsa2_depth_batch", "gcsa2_sv_batch",
    "gcsa2_rmq_batch", "gcsa2_locate_max", "gcsa2_locate_max_batch", "gcsa2_locate_max_into", "gcsa2_sample_range_batch", "gcsa2_sample_batch",
    "gcsa2_sampled_positions", "gcsa2_sigma", "gcsa2_fast_chars", "gcsa2_alphabet", "gcsa2_derive_comp2char",
    "gcsa2_lcp_size", "gcsa2_lcp_values", "gcsa2_lcp_levels", "gcsa2_lcp_branching",
    "gcsa2_lcp_access_batch",
    "gcsa2_group_create", "gcsa2_group_destroy", "gcsa2_group_size", "gcsa2_group_index",
    "gcsa2_group_find_batch", "gcsa2_group_find_device", "gcsa2_group_uses_rccl",
    "gcsa2_group_match_stats_device", "gcsa2_group_locate_device", "gcsa2_comm_match_stats", "gcsa2_comm_locate",
    "gcsa2_comm_unique_id", "gcsa2_comm_create", "gcsa2_comm_create_custom", "gcsa2_comm_destroy", "gcsa2_comm_rank", "gcsa2_comm_world", "gcsa2_comm_rccl_ranks", "gcsa2_comm_gather",
    "gcsa2_pack_ranges32_device", "gcsa2_unpack_ranges32_device", "gcsa2_pack_ranges40_device", "gcsa2_unpack_ranges40_device", "gcsa2_wire48_bytes", "gcsa2_mailbox_stats", "gcsa2_pack_ranges48_device", "gcsa2_unpack_ranges48_device", "gcsa2_count_kmers", "gcsa2_compare_kmers", "gcsa2_compare_kmers_records", "gcsa2_match_stats_batch", "gcsa2_match_stats_device", "gcsa2_match_stats_device_variant", "gcsa2_match_stats_device_sized", "gcsa2_match_stats_profile_device", "gcsa2_match_breaks_device", "gcsa2_match_breaks_batch", "gcsa2_mem_hits_device", "gcsa2_mem_hits_batch",
    "gcsa2_match_breaks_bounded_device", "gcsa2_match_breaks_bounded_batch", "gcsa2_mem_hits_bounded_device", "gcsa2_mem_hits_bounded_batch", "gcsa2_sub_mem_hits_device", "gcsa2_sub_mem_hits_batch",
    "gcsa2_extend_device", "gcsa2_extend_batch", "gcsa2_kmer_windows_device", "gcsa2_kmer_windows_batch",
    "gcsa2_kmer_hits_device", "gcsa2_kmer_hits_batch",
    "gcsa2_minimizers_device", "gcsa2_minimizers_batch", "gcsa2_minimizer_hits_device", "gcsa2_minimizer_hits_batch",
    "gcsa2_capped_seeds_device", "gcsa2_capped_seeds_batch",
    "gcsa2_kmer_support_device", "gcsa2_kmer_support_batch", "gcsa2_seed_support_device",
    "gcsa2_kmer_spectrum", "gcsa2_list_kmers", "gcsa2_index_kmer_support_device",
    "gcsa2_kmer_classes_device", "gcsa2_kmer_classes_batch", "gcsa2_seed_classes_device",
    "gcsa2_kmer_top_classes_device", "gcsa2_kmer_top_classes_batch", "gcsa2_seed_top_classes_device",
    "gcsa2_seed_clusters_device", "gcsa2_kmer_clusters_device", "gcsa2_minimizer_clusters_device", "gcsa2_kmer_clusters_batch",
    "gcsa2_minimizer_clusters_batch",
    "gcsa2_host_view_save", "gcsa2_host_view_load", "gcsa2_host_view_get", "gcsa2_host_view_free",
    "gcsa2_index_create_from_file", "gcsa2_host_view_load_gcsa", "gcsa2_index_create_from_gcsa",
    "gcsa2_host_view_parse_gcsa", "gcsa2_host_view_parse_lcp", "gcsa2_host_view_serialize_gcsa", "gcsa2_host_view_serialize_lcp",
    "gcsa2_lcp_create",
]


SINK = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_uint64)     # gcsa2_sink


class Gcsa2Error(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"gcsa2_hip: {STATUS.get(code, code)}: {message}")
        self.code = code


_lib = None


def load_library():
    """dlopen libgcsa2_hip.so.  When torch is installed it is imported first so that both share
    the one HIP runtime already mapped into the process (same soname, libamdhip64.so.7)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise Gcsa2Error(-2, f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
    try:
        import torch  # noqa: F401  (plumbing only: one HIP runtime per process)
        # ... and one RCCL: the gather entry points bind RCCL at run time (csrc/comm.hpp) and are pointed at
        # the copy torch ships and loads for its own "nccl" backend, when there is one
        bundled = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
        if os.path.exists(bundled):
            os.environ.setdefault("GCSA2_RCCL_LIB", bundled)
    except Exception:
        pass
    L = C.CDLL(LIB_PATH)
    vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int
    L.gcsa2_last_error.restype = C.c_char_p
    L.gcsa2_index_create.argtypes = [C.POINTER(HostView), i32, C.POINTER(vp)]
    L.gcsa2_index_set_tables.argtypes = [vp, i32, i32, i32]
    L.gcsa2_index_trim.argtypes = [vp]
    L.gcsa2_index_set_pipeline.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.gcsa2_index_destroy.argtypes = [vp]
    L.gcsa2_index_destroy.restype = None
    for name in ("gcsa2_size", "gcsa2_edge_count", "gcsa2_order", "gcsa2_sample_count",
                 "gcsa2_sample_bits", "gcsa2_device_bytes", "gcsa2_block_bits", "gcsa2_find_block_bytes", "gcsa2_kmer_table_k", "gcsa2_locate_table_bytes", "gcsa2_jump_table_bytes", "gcsa2_pair_block_bytes",
                 "gcsa2_sampled_positions", "gcsa2_sigma", "gcsa2_fast_chars", "gcsa2_lcp_size",
                 "gcsa2_lcp_values", "gcsa2_lcp_levels", "gcsa2_lcp_branching"):
        getattr(L, name).restype = u64
        getattr(L, name).argtypes = [vp]
    L.gcsa2_jump_mid.argtypes = [vp]
    L.gcsa2_jump_mid_default.argtypes = [u64, i32]
    L.gcsa2_jump_branch.argtypes = [vp]
    L.gcsa2_jump_branch_default.argtypes = [u64, i32]
    L.gcsa2_device.argtypes = [vp]
    L.gcsa2_find_batch.argtypes = [vp, u8p, u64p, u64, u64p]
    L.gcsa2_find_device.argtypes = [vp, vp, vp, u64, vp, vp]
    L.gcsa2_find_batch_packed.argtypes = [vp, u64p, u64, u64, u64p]
    L.gcsa2_find_packed_device.argtypes = [vp, vp, u64, u64, vp, vp]
    L.gcsa2_find_stats_device.argtypes = [vp, vp, vp, u64, vp, vp, vp]
    L.gcsa2_find_device_variant.argtypes = [vp, i32, vp, vp, u64, vp, vp]
    L.gcsa2_lf_batch.argtypes = [vp, u64p, u8p, u64, u64p]
    L.gcsa2_lf_device.argtypes = [vp, vp, vp, u64, vp, vp]
    L.gcsa2_lf_node_batch.argtypes = [vp, u64p, u64, u64p]
    L.gcsa2_char_range.argtypes = [vp, C.c_uint8, u64p, u64p]
    L.gcsa2_lf_all_batch.argtypes = [vp, u64p, u64, i32, u64p]
    L.gcsa2_count_batch.argtypes = [vp, u64p, u64, u64p]
    L.gcsa2_count_device.argtypes = [vp, vp, u64, vp, vp]
    L.gcsa2_locate_run.argtypes = [vp, u64p, u64, i32, u64p, C.POINTER(vp)]
    L.gcsa2_locate_fetch.argtypes = [vp, u64p, u64]
    L.gcsa2_locate_discard.argtypes = [vp]
    L.gcsa2_locate_discard.restype = None
    L.gcsa2_locate_device.argtypes = [vp, vp, u64, i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                                      u64p, vp]
    L.gcsa2_locate_into.argtypes = [vp, vp, u64, i32, vp, vp, u64, u64p, vp]
    L.gcsa2_parent_batch.argtypes = [vp, u64p, u64, vp]
    L.gcsa2_parent_device.argtypes = [vp, vp, u64, vp, vp]
    L.gcsa2_depth_batch.argtypes = [vp, u64p, u64, u64p]
    L.gcsa2_sv_batch.argtypes = [vp, i32, u64p, u64, u64p]
    L.gcsa2_rmq_batch.argtypes = [vp, u64p, u64, u64p]
    L.gcsa2_locate_max.argtypes = [vp, u64, u64, u64, u64p, u64, u64p]
    L.gcsa2_locate_max_batch.argtypes = [vp, u64p, u64, u64, u64p, u64p, u64, u64p]
    L.gcsa2_locate_max_into.argtypes = [vp, vp, u64, u64, vp, vp, u64, u64p, vp]
    L.gcsa2_sample_range_batch.argtypes = [vp, u64p, u64, u64p]
    L.gcsa2_sample_batch.argtypes = [vp, u64p, u64, u64p, u8p]
    L.gcsa2_alphabet.argtypes = [vp, u8p, u64p]
    L.gcsa2_alphabet.restype = None
    L.gcsa2_lcp_access_batch.argtypes = [vp, u64p, u64, u64p]
    L.gcsa2_count_kmers.argtypes = [vp, u64, i32, i32, u64p]
    L.gcsa2_compare_kmers.argtypes = [vp, vp, u64, i32, i32, u64p]
    L.gcsa2_compare_kmers_records.argtypes = [vp, vp, u64, i32, i32, u64p, u64p, u64, u64p, u64]
    L.gcsa2_host_view_save.argtypes = [C.POINTER(HostView), C.c_char_p]
    L.gcsa2_host_view_load.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.gcsa2_host_view_get.argtypes = [vp]
    L.gcsa2_host_view_get.restype = C.POINTER(HostView)
    L.gcsa2_host_view_free.argtypes = [vp]
    L.gcsa2_host_view_free.restype = None
    L.gcsa2_index_create_from_file.argtypes = [C.c_char_p, i32, C.POINTER(vp)]
    L.gcsa2_host_view_load_gcsa.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(vp)]
    L.gcsa2_index_create_from_gcsa.argtypes = [C.c_char_p, C.c_char_p, i32, C.POINTER(vp)]
    L.gcsa2_host_view_parse_gcsa.argtypes = [vp, u64, u64p, C.POINTER(vp)]
    L.gcsa2_host_view_parse_lcp.argtypes = [vp, u64, u64p, C.POINTER(vp)]
    L.gcsa2_host_view_serialize_gcsa.argtypes = [C.POINTER(HostView), SINK, vp, u64p]
    L.gcsa2_host_view_serialize_lcp.argtypes = [C.POINTER(HostView), SINK, vp, u64p]
    L.gcsa2_lcp_create.argtypes = [C.POINTER(HostView), i32, C.POINTER(vp)]
    L.gcsa2_match_stats_batch.argtypes = [vp, u8p, u64p, u64, vp, u64p, u64p]
    L.gcsa2_match_stats_device.argtypes = [vp, vp, vp, u64, vp, vp, vp, vp]
    L.gcsa2_match_stats_device_variant.argtypes = [vp, C.c_int, vp, vp, u64, vp, vp, vp, vp]
    L.gcsa2_match_stats_device_sized.argtypes = [vp, C.c_int, vp, vp, u64, u64, vp, vp, vp, vp]
    L.gcsa2_match_stats_profile_device.argtypes = [vp, vp, vp, u64, u64, vp, vp, vp, vp, vp]
    L.gcsa2_match_breaks_batch.argtypes = [vp, u8p, u64p, u64, u64, u64p, vp, u64, u64p, vp, vp]
    L.gcsa2_match_breaks_device.argtypes = [vp, vp, vp, u64, u64, i32, u64, vp, vp, u64, u64p, vp, vp, vp]
    L.gcsa2_mem_hits_device.argtypes = [vp, vp, vp, u64, u64, u64, u64, i32, vp, vp, u64, u64p, vp, vp, u64, u64p, vp]
    L.gcsa2_mem_hits_batch.argtypes = [vp, u8p, u64p, u64, u64, u64, i32, vp, vp, u64, u64p, vp, vp, u64, u64p]
    L.gcsa2_match_breaks_bounded_batch.argtypes = [vp, u8p, u64p, u64, u64, u64, u64p, vp, u64, u64p, vp, vp]
    L.gcsa2_match_breaks_bounded_device.argtypes = [vp, vp, vp, u64, u64, i32, u64, u64, vp, vp, u64, u64p, vp, vp, vp]
    L.gcsa2_mem_hits_bounded_device.argtypes = [vp, vp, vp, u64, u64, u64, u64, u64, i32, vp, vp, u64, u64p, vp, vp, u64, u64p, vp]
    L.gcsa2_mem_hits_bounded_batch.argtypes = [vp, u8p, u64p, u64, u64, u64, u64, i32, vp, vp, u64, u64p, vp, vp, u64, u64p]
    L.gcsa2_sub_mem_hits_device.argtypes = [vp, vp, vp, u64, u64, vp, vp, u64, u64, u64, u64, i32, vp, vp, u64, u64p, vp, vp, u64, u64p, vp]
    L.gcsa2_sub_mem_hits_batch.argtypes = [vp, u8p, u64p, u64, u64p, vp, u64, u64, u64, u64, i32, vp, vp, u64, u64p, vp, vp, u64, u64p]
    L.gcsa2_extend_device.argtypes = [vp, vp, vp, u64, vp, u64, vp, vp]
    L.gcsa2_extend_batch.argtypes = [vp, u8p, u64p, u64, vp, u64, vp]
    L.gcsa2_kmer_windows_device.argtypes = [vp, vp, vp, u64, u64, u64, C.c_int, vp, vp, vp, vp, u64, u64p, vp]
    L.gcsa2_kmer_windows_batch.argtypes = [vp, u8p, u64p, u64, u64, u64, C.c_int, vp, vp, vp, vp, u64, u64p]
    L.gcsa2_kmer_hits_device.argtypes = [vp, vp, vp, u64, u64, u64, u64, C.c_int, vp, vp, vp, u64, u64p, vp, vp, u64, u64p, vp]
    L.gcsa2_kmer_hits_batch.argtypes = [vp, u8p, u64p, u64, u64, u64, u64, C.c_int, vp, vp, vp, u64, u64p, vp, vp, u64, u64p]
    L.gcsa2_minimizers_device.argtypes = [vp, vp, vp, u64, u64, u64, u64, vp, vp, u64, u64p, vp]
    L.gcsa2_minimizers_batch.argtypes = [vp, u8p, u64p, u64, u64, u64, u64, vp, vp, u64, u64p]
    L.gcsa2_minimizer_hits_device.argtypes = [vp, vp, vp, u64, u64, u64, u64, u64, C.c_int, vp, vp, vp, u64, u64p, vp, vp, u64, u64p, vp]
    L.gcsa2_minimizer_hits_batch.argtypes = [vp, u8p, u64p, u64, u64, u64, u64, u64, C.c_int, vp, vp, vp, u64, u64p, vp, vp, u64, u64p]
    L.gcsa2_kmer_support_device.argtypes = [vp, vp, vp, u64, u64, u64, u64, u64, C.c_int, vp, u64, vp, vp]
    L.gcsa2_kmer_support_batch.argtypes = [vp, u8p, u64p, u64, u64, u64, u64, u64, C.c_int, vp, u64, vp]
    L.gcsa2_seed_support_device.argtypes = [vp, vp, u64, vp, u64, u64, C.c_int, vp, u64, vp, vp]
    L.gcsa2_kmer_spectrum.argtypes = [vp, u64, i32, i32, i32, vp, u64, vp]
    L.gcsa2_list_kmers.argtypes = [vp, u64, i32, i32, i32, u64, u64, vp, u64, u64p]
    L.gcsa2_index_kmer_support_device.argtypes = [vp, u64, i32, i32, u64, u64, C.c_int, vp, u64, vp, vp]
    L.gcsa2_kmer_classes_device.argtypes = [vp, vp, vp, u64, u64, u64, u64, u64, C.c_int, vp, u64, u64, vp, vp, vp, vp]
    L.gcsa2_kmer_classes_batch.argtypes = [vp, u8p, u64p, u64, u64, u64, u64, u64, C.c_int, vp, u64, u64, vp, vp, vp]
    L.gcsa2_seed_classes_device.argtypes = [vp, vp, u64, vp, u64, vp, u64, u64, C.c_int, vp, u64, u64, vp, vp, vp, vp]
    L.gcsa2_kmer_top_classes_device.argtypes = [vp, vp, vp, u64, u64, u64, u64, u64, C.c_int, vp, u64, u64, u64, vp, vp, vp, vp]
    L.gcsa2_kmer_top_classes_batch.argtypes = [vp, u8p, u64p, u64, u64, u64, u64, u64, C.c_int, vp, u64, u64, u64, vp, vp, vp]
    L.gcsa2_seed_top_classes_device.argtypes = [vp, vp, u64, vp, u64, vp, u64, u64, C.c_int, vp, u64, u64, u64, vp, vp, vp, vp]
    L.gcsa2_seed_clusters_device.argtypes = [vp, vp, u64, vp, u64, vp, vp, u64, u64, vp, u64, u64, u64, vp, vp, vp, vp]
    L.gcsa2_kmer_clusters_device.argtypes = [vp, vp, vp, u64, u64, u64, u64, C.c_int, u64, vp, u64, u64, u64, vp, vp, vp, vp]
    L.gcsa2_minimizer_clusters_device.argtypes = [vp, vp, vp, u64, u64, u64, u64, u64, C.c_int, u64, vp, u64, u64, u64, vp, vp, vp, vp]
    L.gcsa2_kmer_clusters_batch.argtypes = [vp, u8p, u64p, u64, u64, u64, u64, C.c_int, u64, vp, u64, u64, u64, vp, vp, vp]
    L.gcsa2_minimizer_clusters_batch.argtypes = [vp, u8p, u64p, u64, u64, u64, u64, u64, C.c_int, u64, vp, u64, u64, u64, vp, vp, vp]
    declare_chain_calls(L)
    declare_strand_calls(L)
    declare_pair_calls(L)
    L.gcsa2_capped_seeds_device.argtypes = [vp, vp, vp, u64, u64, u64, u64, u64, C.c_int, vp, vp, u64, u64p, vp, vp, u64, u64p, vp]
    L.gcsa2_capped_seeds_batch.argtypes = [vp, u8p, u64p, u64, u64, u64, u64, u64, C.c_int, vp, vp, u64, u64p, vp, vp, u64, u64p]
    L.gcsa2_group_create.argtypes = [C.POINTER(HostView), C.POINTER(i32), i32, C.POINTER(vp)]
    L.gcsa2_group_destroy.argtypes = [vp]
    L.gcsa2_group_destroy.restype = None
    L.gcsa2_group_size.argtypes = [vp]
    L.gcsa2_group_index.argtypes = [vp, i32]
    L.gcsa2_group_index.restype = vp
    L.gcsa2_group_find_batch.argtypes = [vp, u8p, u64p, u64, u64p]
    L.gcsa2_group_find_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), u64p, vp]
    L.gcsa2_group_uses_rccl.argtypes = [vp]
    L.gcsa2_group_match_stats_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), u64p, u64p, vp, vp, vp]
    L.gcsa2_group_locate_device.argtypes = [vp, C.POINTER(vp), u64p, i32, vp, C.POINTER(vp), C.POINTER(vp), u64p]
    L.gcsa2_comm_match_stats.argtypes = [vp, vp, vp, vp, u64p, u64p, i32, vp, vp, vp, vp]
    L.gcsa2_comm_locate.argtypes = [vp, vp, vp, u64p, i32, i32, vp, C.POINTER(vp), C.POINTER(vp), u64p, vp]
    L.gcsa2_comm_unique_id.argtypes = [u8p]
    L.gcsa2_comm_create.argtypes = [u8p, i32, i32, i32, C.POINTER(vp)]
    L.gcsa2_comm_create_custom.argtypes = [i32, i32, i32, vp, vp, C.POINTER(vp)]
    L.gcsa2_comm_destroy.argtypes = [vp]
    L.gcsa2_comm_destroy.restype = None
    L.gcsa2_comm_rank.argtypes = [vp]
    L.gcsa2_comm_world.argtypes = [vp]
    L.gcsa2_comm_rccl_ranks.argtypes = [vp, C.POINTER(C.c_int)]
    L.gcsa2_comm_gather.argtypes = [vp, vp, u64p, vp, i32, vp]
    L.gcsa2_pack_ranges32_device.argtypes = [vp, u64, vp, vp]
    L.gcsa2_unpack_ranges32_device.argtypes = [vp, u64, vp, vp]
    L.gcsa2_pack_ranges40_device.argtypes = [vp, u64, vp, vp]
    L.gcsa2_unpack_ranges40_device.argtypes = [vp, u64, vp, vp]
    L.gcsa2_mailbox_stats.argtypes = [vp, u64p, u64p]
    L.gcsa2_wire48_bytes.argtypes = [u64, u64]
    L.gcsa2_wire48_bytes.restype = u64
    L.gcsa2_pack_ranges48_device.argtypes = [vp, u64, vp, u64, vp]
    L.gcsa2_unpack_ranges48_device.argtypes = [vp, u64, u64, vp, vp, vp]
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise Gcsa2Error(rc, load_library().gcsa2_last_error().decode(errors="replace"))


def device_count():
    rc = load_library().gcsa2_device_count()
    if rc < 0:
        _check(rc)
    return rc


def jump_mid_default(nodes, pair_blocks):
    """The jump_mid that index creation chooses for an image of `nodes` path nodes with or without pair blocks, when
    GCSA2_JUMP_MID does not override it (gcsa2_jump_mid_default)."""
    return int(load_library().gcsa2_jump_mid_default(int(nodes), 1 if pair_blocks else 0))


def jump_branch_default(nodes, pair_blocks):
    """1 when index creation writes branch records into the jump table of an image of `nodes` path nodes with or without
    pair blocks, when GCSA2_JUMP_BRANCH does not override it (gcsa2_jump_branch_default)."""
    return int(load_library().gcsa2_jump_branch_default(int(nodes), 1 if pair_blocks else 0))


def _p64(a):
    return a.ctypes.data_as(u64p)


def _p8(a):
    return a.ctypes.data_as(u8p)


def _ranges(r):
    r = np.ascontiguousarray(r, dtype=np.uint64)
    if r.ndim == 1:
        r = r.reshape(-1, 2)
    return r


class Range:
    """`gcsa::Range` (reference include/gcsa/utils.h:84-117)."""

    @staticmethod
    def length(r):
        return (int(r[1]) + 1 - int(r[0])) & UNKNOWN

    @staticmethod
    def empty(r):
        return ((int(r[0]) + 1) & UNKNOWN) > ((int(r[1]) + 1) & UNKNOWN)

    @staticmethod
    def empty_range():
        return (1, 0)


class Node:
    """`gcsa::Node` (reference include/gcsa/support.h:443-471): id << 11 | rc << 10 | offset."""
    OFFSET_BITS = 10
    ID_OFFSET = 11

    @staticmethod
    def encode(node_id, offset=0, rc=False):
        return (node_id << 11) | (int(bool(rc)) << 10) | offset

    @staticmethod
    def id(node):
        return int(node) >> 11

    @staticmethod
    def rc(node):
        return bool((int(node) >> 10) & 1)

    @staticmethod
    def offset(node):
        return int(node) & 1023


def save_host_view(index_arrays, path, **view_kwargs):
    """Write the G2HV container file of an index (host only)."""
    holder = make_host_view(index_arrays, **view_kwargs)
    _check(load_library().gcsa2_host_view_save(holder.ref(), os.fsencode(path)))


class LoadedHostView:
    """A G2HV file, or a `.gcsa` (+ `.lcp`) pair, read back into host memory (host only); `.view` is
    the ctypes HostView."""

    def __init__(self, path, lcp_path=None):
        self._L = load_library()
        h = C.c_void_p()
        if os.fspath(path).endswith(".gcsa"):
            _check(self._L.gcsa2_host_view_load_gcsa(os.fsencode(path), os.fsencode(lcp_path) if lcp_path else None, C.byref(h)))
        else:
            _check(self._L.gcsa2_host_view_load(os.fsencode(path), C.byref(h)))
        self._h = h
        self.view = self._L.gcsa2_host_view_get(h).contents

    def close(self):
        if getattr(self, "_h", None):
            self._L.gcsa2_host_view_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GCSA(ChainCalls, StrandCalls, PairCalls):
    """Device-resident index with the reference's query methods.

    Scalar methods (`find`, `LF`, `count`, `locate`, ...) are one-element batches of the batched
    ones; the batched ones take / return numpy arrays.  `*_device` methods take raw device
    pointers (ints) and a stream pointer and only enqueue work."""

    def __init__(self, index_arrays, device=0, **view_kwargs):
        L = load_library()
        h = C.c_void_p()
        if isinstance(index_arrays, (str, bytes, os.PathLike)):      # a G2HV container or a `.gcsa` file (+ `.lcp` beside it)
            path = os.fspath(index_arrays)
            path = path.decode() if isinstance(path, bytes) else path
            if path.endswith(".gcsa"):     # GCSA::EXTENSION / LCPArray::EXTENSION (gcsa.h:63, lcp.h:110)
                # query_gcsa names the pair base.gcsa + base.lcp (benchmark/query_gcsa.cpp:53-63), vg base.gcsa + base.gcsa.lcp
                beside = [p for p in (path[:-5] + ".lcp", path + ".lcp") if os.path.exists(p)]
                lcp = view_kwargs.pop("lcp_path", beside[0] if beside else None)
                _check(L.gcsa2_index_create_from_gcsa(os.fsencode(path), os.fsencode(lcp) if lcp else None, device, C.byref(h)))
            else:
                _check(L.gcsa2_index_create_from_file(os.fsencode(path), device, C.byref(h)))
            self._h, self._L = h, L
            self.sigma = int(L.gcsa2_sigma(h))
            self.fast_chars = int(L.gcsa2_fast_chars(h))
            self.char2comp = np.zeros(256, dtype=np.uint8)
            L.gcsa2_alphabet(h, _p8(self.char2comp), None)
            return
        holder = make_host_view(index_arrays, **view_kwargs)
        _check(L.gcsa2_index_create(holder.ref(), device, C.byref(h)))
        self._h = h
        self._L = L
        self.char2comp = np.asarray(index_arrays.char2comp, dtype=np.uint8).copy()
        self.sigma = int(index_arrays.sigma)
        self.fast_chars = int(index_arrays.fast_chars)

    def close(self):
        if getattr(self, "_h", None):
            self._L.gcsa2_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    # header accessors (gcsa.h:137-148)
    def size(self):
        return int(self._L.gcsa2_size(self._h))

    def empty(self):
        return self.size() == 0

    def edgeCount(self):
        return int(self._L.gcsa2_edge_count(self._h))

    def order(self):
        return int(self._L.gcsa2_order(self._h))

    def sampleCount(self):
        return int(self._L.gcsa2_sample_count(self._h))

    def sampleBits(self):
        return int(self._L.gcsa2_sample_bits(self._h))

    def device_bytes(self):
        return int(self._L.gcsa2_device_bytes(self._h))

    def block_bits(self):
        return int(self._L.gcsa2_block_bits(self._h))

    # ---- find ---------------------------------------------------------------------------
    def find_batch(self, patterns, offsets, out=None):
        """`out`: an (nq, 2) uint64 array to receive the ranges (a caller that reuses its result buffer avoids the page
        faults of a fresh one, which cost as much as the batch itself at 10 M queries)."""
        patterns = np.ascontiguousarray(patterns, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        nq = offsets.shape[0] - 1
        if out is None:
            out = np.zeros((nq, 2), dtype=np.uint64)
        assert out.dtype == np.uint64 and out.shape == (nq, 2) and out.flags["C_CONTIGUOUS"]
        _check(self._L.gcsa2_find_batch(self._h, _p8(patterns), _p64(offsets), nq, _p64(out)))
        return out

    def find(self, pattern):
        data, off = concat_patterns([pattern])
        r = self.find_batch(data, off)[0]
        return (int(r[0]), int(r[1]))

    def find_batch_packed(self, codes, pattern_length, out=None):
        """find() of patterns of one length given as 2-bit codes (pack_kmers): (nq, W) uint64, W = ceil(pattern_length / 32)."""
        codes = np.ascontiguousarray(codes, dtype=np.uint64)
        words = (int(pattern_length) + 31) // 32
        nq = codes.size // words
        if out is None:
            out = np.zeros((nq, 2), dtype=np.uint64)
        assert out.dtype == np.uint64 and out.shape == (nq, 2) and out.flags["C_CONTIGUOUS"]
        _check(self._L.gcsa2_find_batch_packed(self._h, _p64(codes), int(pattern_length), nq, _p64(out)))
        return out

    def find_packed_device(self, d_codes, pattern_length, nq, d_ranges, stream=0):
        _check(self._L.gcsa2_find_packed_device(self._h, d_codes, int(pattern_length), nq, d_ranges, stream))

    def find_device(self, d_patterns, d_offsets, nq, d_ranges, stream=0):
        _check(self._L.gcsa2_find_device(self._h, d_patterns, d_offsets, nq, d_ranges, stream))

    def find_device_variant(self, variant, d_patterns, d_offsets, nq, d_ranges, stream=0):
        _check(self._L.gcsa2_find_device_variant(self._h, variant, d_patterns, d_offsets, nq, d_ranges, stream))

    def jump_table_bytes(self):
        return int(self._L.gcsa2_jump_table_bytes(self._h))

    def jump_mid(self):
        """Steps behind the middle node slot of this image's jump entries, 2 or 6 (gcsa2_jump_mid)."""
        return int(self._L.gcsa2_jump_mid(self._h))

    def jump_branch(self):
        """1 when this image's jump table holds branch records, else 0 (gcsa2_jump_branch)."""
        return int(self._L.gcsa2_jump_branch(self._h))

    def set_tables(self, pair_blocks=-1, kmer_k=-1, locate_table=-1):
        """Drop (0) / build (1) / leave (-1) the pair blocks and the locate table, resize the k-mer seed table (0 drops it):
        gcsa2_index_set_tables.  Results of every query stay the same; no queries may run on the handle meanwhile."""
        _check(self._L.gcsa2_index_set_tables(self._h, int(pair_blocks), int(kmer_k), int(locate_table)))

    def trim(self):
        """Give back the host pipeline, the staging objects and the scratch pool of this handle (gcsa2_index_trim)."""
        _check(self._L.gcsa2_index_trim(self._h))

    def set_pipeline(self, lanes=0, chunk_log2=0, blocking=-1):
        """Shape of the host pipeline of find_batch / find_batch_packed (gcsa2_index_set_pipeline; 0 leaves a value)."""
        _check(self._L.gcsa2_index_set_pipeline(self._h, int(lanes), int(chunk_log2), int(blocking)))

    def pair_block_bytes(self):
        return int(self._L.gcsa2_pair_block_bytes(self._h))

    def mailbox_stats(self):
        """(scalar calls answered by the resident wavefront, launches of it): gcsa2_mailbox_stats."""
        calls, launches = C.c_uint64(0), C.c_uint64(0)
        _check(self._L.gcsa2_mailbox_stats(self._h, C.byref(calls), C.byref(launches)))
        return int(calls.value), int(launches.value)

    def locate_table_bytes(self):
        return int(self._L.gcsa2_locate_table_bytes(self._h))

    def kmer_table_k(self):
        return int(self._L.gcsa2_kmer_table_k(self._h))

    def find_block_bytes(self):
        return int(self._L.gcsa2_find_block_bytes(self._h))

    def find_stats_device(self, d_patterns, d_offsets, nq, d_ranges, d_stats, stream=0):
        _check(self._L.gcsa2_find_stats_device(self._h, d_patterns, d_offsets, nq, d_ranges, d_stats, stream))

    # ---- LF -----------------------------------------------------------------------------
    def lf_batch(self, ranges, comps):
        ranges = _ranges(ranges)
        comps = np.ascontiguousarray(comps, dtype=np.uint8)
        out = np.zeros_like(ranges)
        _check(self._L.gcsa2_lf_batch(self._h, _p64(ranges), _p8(comps), ranges.shape[0], _p64(out)))
        return out

    def extend_batch(self, patterns, offsets, states):
        """The backward search continued from caller ranges (gcsa2_extend_batch): `states` is an (n, 5) uint64 array of
        (pattern, begin, end, sp, ep) -- continue from (sp, ep) over P[begin, end) of pattern `pattern`, last character first.
        Returns (n, 5) uint64 rows (matched, sp, ep, last_sp, last_ep): the steps that left a non-empty range, the range the
        reference's loop ends with, and the last non-empty range.  An invalid state has matched = 2^64 - 1 and its start range."""
        patterns = np.ascontiguousarray(patterns, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        states = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1, 5)
        out = np.zeros_like(states)
        _check(self._L.gcsa2_extend_batch(self._h, _p8(patterns), _p64(offsets), max(offsets.shape[0], 1) - 1, states.ctypes.data,
                                          states.shape[0], out.ctypes.data))
        return out

    def extend_device(self, d_patterns, d_offsets, n_patterns, d_states, n_states, d_out, stream=0):
        """gcsa2_extend_device on caller-owned device buffers: enqueues on `stream` and returns."""
        _check(self._L.gcsa2_extend_device(self._h, d_patterns, d_offsets, n_patterns, d_states, n_states, d_out, stream))

    def kmer_windows_batch(self, patterns, offsets, k, stride=1, counts=False, ranges=True, profiles=True, occurrences=False):
        """find() (and count()) of every window P_q[j stride, j stride + k) of every read of a batch in host memory
        (gcsa2_kmer_windows_batch).  Returns (window_offsets, profiles, ranges, counts): window_offsets (reads + 1) is the
        exclusive prefix sum of the windows per read, profiles (reads, 4) holds (windows, found, nodes, occurrences) per read,
        ranges (windows, 2) is find() of each window and counts (windows) its count(); None for what was not asked.
        `counts` also fills profiles' occurrences; `occurrences=True` does that without the counts array.  Either needs the
        counters."""
        patterns = np.ascontiguousarray(patterns, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = max(offsets.shape[0], 1) - 1
        k, stride = int(k), int(stride)
        flags = KMER_COUNTS if (counts or occurrences) else 0
        total = 0
        if n > 0 and k > 0 and stride > 0 and (ranges or counts):          # the sizes of the per-window arrays (the call checks the rest)
            lens = np.diff(offsets.astype(np.int64))
            total = int(np.where(lens >= k, (lens - k) // stride + 1, 0).sum())
        woff = np.zeros(n + 1, dtype=np.uint64)
        prof = np.zeros((n, 4), dtype=np.uint64) if profiles else None
        rng = np.zeros((total, 2), dtype=np.uint64) if ranges else None
        cnt = np.zeros(total, dtype=np.uint64) if counts else None
        needed = C.c_uint64()
        rc = self._L.gcsa2_kmer_windows_batch(self._h, _p8(patterns), _p64(offsets), n, k, stride, flags, woff.ctypes.data,
                                              None if prof is None else prof.ctypes.data, None if rng is None else rng.ctypes.data,
                                              None if cnt is None else cnt.ctypes.data, total, C.byref(needed))
        if rc != 0:
            err = Gcsa2Error(rc, self._L.gcsa2_last_error().decode(errors="replace"))
            err.needed = needed.value
            raise err
        return woff, prof, rng, cnt

    def kmer_windows_device(self, d_patterns, d_offsets, n_patterns, k, stride, flags, d_window_offsets, d_profiles, d_ranges, d_counts,
                            capacity, stream=0):
        """gcsa2_kmer_windows_device on caller-owned device buffers (raw pointers; 0 / None for an output that is not wanted):
        d_window_offsets n_patterns + 1 u64, d_profiles n_patterns records of four u64, d_ranges / d_counts `capacity` windows.
        Complete on return.  Returns the number of windows; raises Gcsa2Error with `.needed` = that number otherwise
        (BUFFER_TOO_SMALL: more than `capacity`)."""
        needed = C.c_uint64()
        rc = self._L.gcsa2_kmer_windows_device(self._h, d_patterns, d_offsets, n_patterns, int(k), int(stride), int(flags), d_window_offsets or None,
                                               d_profiles or None, d_ranges or None, d_counts or None, int(capacity), C.byref(needed), stream)
        if rc != 0:
            err = Gcsa2Error(rc, self._L.gcsa2_last_error().decode(errors="replace"))
            err.needed = needed.value
            raise err
        return needed.value

    def kmer_hits_batch(self, patterns, offsets, k, stride=1, hit_max=0, sample=False, profiles=False, out=None):
        """The k-mers of every read that occur, as seeds with counts and positions (gcsa2_kmer_hits_batch): (seed_offsets
        (reads + 1), seeds (total, 5) = {position, length = k, sp, ep, count}, hit_offsets (total + 1), hits[, profiles (reads,
        4)]).  The seeds of a read are its windows P_q[j stride, j stride + k) with a non-empty find(), in window order; a seed's
        hits follow mem_hits_batch's rules (hit_max, sample).  The rows of `seeds` are MEM records: sub_mem_hits_batch takes them
        as they are.  The buffers are sized from a first refusal.  `out` = (seed_offsets, seeds, hit_offsets, hits) arrays of
        the caller; too small ones raise BUFFER_TOO_SMALL with `needed` = (seeds, hits)."""
        patterns = np.ascontiguousarray(patterns, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = max(offsets.shape[0], 1) - 1
        over = 1 if sample else 0
        prof = np.zeros((n, 4), dtype=np.uint64) if profiles else None
        total_m, total_h = C.c_uint64(), C.c_uint64()

        def call(soff, seeds, hoff, hits):
            assert soff.dtype == np.uint64 and soff.shape[0] >= n + 1 and seeds.dtype == np.uint64 and seeds.flags.c_contiguous
            assert seeds.shape[1] == 5 and hoff.dtype == np.uint64 and hoff.shape[0] >= seeds.shape[0] + 1 and hits.dtype == np.uint64
            return self._L.gcsa2_kmer_hits_batch(self._h, _p8(patterns), _p64(offsets), n, int(k), int(stride), int(hit_max), over,
                                                 None if prof is None else prof.ctypes.data, soff.ctypes.data, seeds.ctypes.data,
                                                 seeds.shape[0], C.byref(total_m), hoff.ctypes.data, hits.ctypes.data, hits.shape[0],
                                                 C.byref(total_h))

        if out is not None:
            soff, seeds, hoff, hits = out
            rc = call(soff, seeds, hoff, hits)
        else:
            mcap, hcap = 0, 0
            soff = np.zeros(n + 1, dtype=np.uint64)
            for _ in range(2):
                seeds = np.zeros((mcap, 5), dtype=np.uint64)
                hoff = np.zeros(mcap + 1, dtype=np.uint64)
                hits = np.zeros(hcap, dtype=np.uint64)
                rc = call(soff, seeds, hoff, hits)
                if rc != STATUS_BUFFER_TOO_SMALL:
                    break
                mcap, hcap = max(mcap, total_m.value), max(hcap, total_h.value)
        if rc == STATUS_BUFFER_TOO_SMALL:
            err = Gcsa2Error(rc, self._L.gcsa2_last_error().decode(errors="replace"))
            err.needed = (total_m.value, total_h.value)
            raise err
        _check(rc)
        m, h = total_m.value, total_h.value
        res = (soff[: n + 1], seeds[:m], hoff[: m + 1], hits[:h])
        return res + (prof,) if profiles else res

    def kmer_hits_device(self, d_patterns, d_offsets, n_patterns, k, stride, hit_max, sample, d_profiles, d_seed_offsets, d_seeds,
                         seed_capacity, d_hit_offsets, d_hits, hit_capacity, stream=0):
        """gcsa2_kmer_hits_device on caller-owned device buffers (raw pointers): d_profiles n_patterns records of four u64 or
        0 / None, d_seed_offsets n_patterns + 1 u64, d_seeds seed_capacity records of five u64, d_hit_offsets seed_capacity + 1
        entries, d_hits hit_capacity values.  `sample`: a bool, or the `over` policy as an int.  Complete on return.  Returns
        (seeds, hits); raises Gcsa2Error (BUFFER_TOO_SMALL, `.needed` = (seeds, hits)) when a buffer is too small."""
        total_m, total_h = C.c_uint64(), C.c_uint64()
        over = sample if isinstance(sample, int) and not isinstance(sample, bool) else (1 if sample else 0)
        rc = self._L.gcsa2_kmer_hits_device(self._h, d_patterns, d_offsets, n_patterns, int(k), int(stride), int(hit_max), over, d_profiles or None,
                                            d_seed_offsets, d_seeds or None, int(seed_capacity), C.byref(total_m), d_hit_offsets, d_hits or None,
                                            int(hit_capacity), C.byref(total_h), stream)
        if rc != 0:
            err = Gcsa2Error(rc, self._L.gcsa2_last_error().decode(errors="replace"))
            err.needed = (total_m.value, total_h.value)
            raise err
        return total_m.value, total_h.value

    def minimizers_batch(self, patterns, offsets, k, w, hash_seed=0, out=None):
        """The (w, k)-minimizers of every read of a batch in host memory (gcsa2_minimizers_batch): (min_offsets (reads + 1),
        minimizers (total, 2) = {position, hash}).  Of every w consecutive valid k-mers of a read the one with the smallest
        (hash, position) is selected, hash = SplitMix64's finaliser of the 2-bit packed k-mer ^ hash_seed; a run of fewer than w
        valid k-mers gives one.  Needs nothing of the index but its alphabet.  The records are sized from a first refusal.
        `out` = (min_offsets, minimizers) arrays of the caller; too small ones raise BUFFER_TOO_SMALL with `needed`."""
        patterns = np.ascontiguousarray(patterns, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = max(offsets.shape[0], 1) - 1
        total = C.c_uint64()

        def call(moff, mins):
            assert moff.dtype == np.uint64 and moff.shape[0] >= n + 1 and mins.dtype == np.uint64 and mins.flags.c_contiguous and mins.shape[1] == 2
            return self._L.gcsa2_minimizers_batch(self._h, _p8(patterns), _p64(offsets), n, int(k), int(w), int(hash_seed), moff.ctypes.data,
                                                  mins.ctypes.data, mins.shape[0], C.byref(total))

        if out is not None:
            moff, mins = out
            rc = call(moff, mins)
        else:
            moff = np.zeros(n + 1, dtype=np.uint64)
            mins = np.zeros((0, 2), dtype=np.uint64)
            rc = call(moff, mins)
            if rc == STATUS_BUFFER_TOO_SMALL and total.value > 0:
                mins = np.zeros((total.value, 2), dtype=np.uint64)
                rc = call(moff, mins)
        if rc == STATUS_BUFFER_TOO_SMALL:
            err = Gcsa2Error(rc, self._L.gcsa2_last_error().decode(errors="replace"))
            err.needed = total.value
            raise err
        _check(rc)
        return moff[: n + 1], mins[: total.value]

    def minimizers_device(self, d_patterns, d_offsets, n_patterns, k, w, hash_seed, d_min_offsets, d_minimizers, capacity, stream=0):
        """gcsa2_minimizers_device on caller-owned device buffers (raw pointers): d_min_offsets n_patterns + 1 u64, d_minimizers
        `capacity` records of two u64 {position, hash} (0 / None with capacity 0: a sizing call).  Complete on return.  Returns
        the number of minimizers; raises Gcsa2Error with `.needed` = that number otherwise (BUFFER_TOO_SMALL: more than
        `capacity`; the offsets are complete then)."""
        needed = C.c_uint64()
        rc = self._L.gcsa2_minimizers_device(self._h, d_patterns, d_offsets, n_patterns, int(k), int(w), int(hash_seed), d_min_offsets,
                                             d_minimizers or None, int(capacity), C.byref(needed), stream)
        if rc != 0:
            err = Gcsa2Error(rc, self._L.gcsa2_last_error().decode(errors="replace"))
            err.needed = needed.value
            raise err
        return needed.value

    def minimizer_hits_batch(self, patterns, offsets, k, w, hash_seed=0, hit_max=0, sample=False, profiles=False, out=None):
        """The minimizers of every read that occur, as seeds with counts and positions (gcsa2_minimizer_hits_batch):
        kmer_hits_batch with the (w, k)-minimizers of minimizers_batch as the windows, in the place of every stride-th one.
        Returns (seed_offsets (reads + 1), seeds (total, 5) = {position, length = k, sp, ep, count}, hit_offsets (total + 1),
        hits[, profiles (reads, 4)]); profiles' windows are the minimizers of the read.  The buffers are sized from a first
        refusal.  `out` = (seed_offsets, seeds, hit_offsets, hits) arrays of the caller; too small ones raise BUFFER_TOO_SMALL
        with `needed` = (seeds, hits)."""
        patterns = np.ascontiguousarray(patterns, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = max(offsets.shape[0], 1) - 1
        over = 1 if sample else 0
        prof = np.zeros((n, 4), dtype=np.uint64) if profiles else None
        total_m, total_h = C.c_uint64(), C.c_uint64()

        def call(soff, seeds, hoff, hits):
            assert soff.dtype == np.uint64 and soff.shape[0] >= n + 1 and seeds.dtype == np.uint64 and seeds.flags.c_contiguous
            assert seeds.shape[1] == 5 and hoff.dtype == np.uint64 and hoff.shape[0] >= seeds.shape[0] + 1 and hits.dtype == np.uint64
            return self._L.gcsa2_minimizer_hits_batch(self._h, _p8(patterns), _p64(offsets), n, int(k), int(w), int(hash_seed), int(hit_max), over,
                                                      None if prof is None else prof.ctypes.data, soff.ctypes.data, seeds.ctypes.data,
                                                      seeds.shape[0], C.byref(total_m), hoff.ctypes.data, hits.ctypes.data, hits.shape[0],
                                                      C.byref(total_h))

        if out is not None:
            soff, seeds, hoff, hits = out
            rc = call(soff, seeds, hoff, hits)
        else:
            mcap, hcap = 0, 0
            soff = np.zeros(n + 1, dtype=np.uint64)
            for _ in range(2):
                seeds = np.zeros((mcap, 5), dtype=np.uint64)
                hoff = np.zeros(mcap + 1, dtype=np.uint64)
                hits = np.zeros(hcap, dtype=np.uint64)
                rc = call(soff, seeds, hoff, hits)
                if rc != STATUS_BUFFER_TOO_SMALL:
                    break
                mcap, hcap = max(mcap, total_m.value), max(hcap, total_h.value)
        if rc == STATUS_BUFFER_TOO_SMALL:
            err = Gcsa2Error(rc, self._L.gcsa2_last_error().decode(errors="replace"))
            err.needed = (total_m.value, total_h.value)
            raise err
        _check(rc)
        m, h = total_m.value, total_h.value
        res = (soff[: n + 1], seeds[:m], hoff[: m + 1], hits[:h])
        return res + (prof,) if profiles else res

    def minimizer_hits_device(self, d_patterns, d_offsets, n_patterns, k, w, hash_seed, hit_max, sample, d_profiles, d_seed_offsets, d_seeds,
                              seed_capacity, d_hit_offsets, d_hits, hit_capacity, stream=0):
        """gcsa2_minimizer_hits_device on caller-owned device buffers (raw pointers), the buffers as for kmer_hits_device.
        `sample`: a bool, or the `over` policy as an int.  Complete on return.  Returns (seeds, hits); raises Gcsa2Error
        (BUFFER_TOO_SMALL, `.needed` = (seeds, hits)) when a buffer is too small."""
        total_m, total_h = C.c_uint64(), C.c_uint64()
        over = sample if isinstance(sample, int) and not isinstance(sample, bool) else (1 if sample else 0)
        rc = self._L.gcsa2_minimizer_hits_device(self._h, d_patterns, d_offsets, n_patterns, int(k), int(w), int(hash_seed), int(hit_max), over,
                                                 d_profiles or None, d_seed_offsets, d_seeds or None, int(seed_capacity), C.byref(total_m),
                                                 d_hit_offsets, d_hits or None, int(hit_capacity), C.byref(total_h), stream)
        if rc != 0:
            err = Gcsa2Error(rc, self._L.gcsa2_last_error().decode(errors="replace"))
            err.needed = (total_m.value, total_h.value)
            raise err
        return total_m.value, total_h.value

    def capped_seeds_batch(self, patterns, offsets, min_length, max_length=0, max_count=1, hit_max=0, sample=False, out=None):
        """The shortest matches of every read that occur at most max_count times, with counts and positions
        (gcsa2_capped_seeds_batch): (seed_offsets (reads + 1), seeds (total, 5) = {position, length, sp, ep, count}, hit_offsets
        (total + 1), hits).  From the end of a read the match is extended until it has min_length characters and count() <=
        max_count, emitted, and the search starts again behind it; max_length (0: none) cuts an attempt short.  The seeds of a
        read do not overlap and come in descending position; a seed's hits follow mem_hits_batch's rules (hit_max, sample).
        The rows of `seeds` are MEM records: sub_mem_hits_batch takes them as they are.  Needs no LCP array.  The buffers are
        sized from a first refusal.  `out` = (seed_offsets, seeds, hit_offsets, hits) arrays of the caller; too small ones
        raise BUFFER_TOO_SMALL with `needed` = (seeds, hits)."""
        patterns = np.ascontiguousarray(patterns, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = max(offsets.shape[0], 1) - 1
        over = 1 if sample else 0
        total_m, total_h = C.c_uint64(), C.c_uint64()

        def call(soff, seeds, hoff, hits):
            assert soff.dtype == np.uint64 and soff.shape[0] >= n + 1 and seeds.dtype == np.uint64 and seeds.flags.c_contiguous
            assert seeds.shape[1] == 5 and hoff.dtype == np.uint64 and hoff.shape[0] >= seeds.shape[0] + 1 and hits.dtype == np.uint64
            return self._L.gcsa2_capped_seeds_batch(self._h, _p8(patterns), _p64(offsets), n, int(min_length), int(max_length), int(max_count),
                                                    int(hit_max), over, soff.ctypes.data, seeds.ctypes.data, seeds.shape[0], C.byref(total_m),
                                                    hoff.ctypes.data, hits.ctypes.data, hits.shape[0], C.byref(total_h))

        if out is not None:
            soff, seeds, hoff, hits = out
            rc = call(soff, seeds, hoff, hits)
        else:
            mcap, hcap = 0, 0
            soff = np.zeros(n + 1, dtype=np.uint64)
            for _ in range(2):
                seeds = np.zeros((mcap, 5), dtype=np.uint64)
                hoff = np.zeros(mcap + 1, dtype=np.uint64)
                hits = np.zeros(hcap, dtype=np.uint64)
                rc = call(soff, seeds, hoff, hits)
                if rc != STATUS_BUFFER_TOO_SMALL:
                    break
                mcap, hcap = max(mcap, total_m.value), max(hcap, total_h.value)
        if rc == STATUS_BUFFER_TOO_SMALL:
            err = Gcsa2Error(rc, self._L.gcsa2_last_error().decode(errors="replace"))
            err.needed = (total_m.value, total_h.value)
            raise err
        _check(rc)
        m, h = total_m.value, total_h.value
        return soff[: n + 1], seeds[:m], hoff[: m + 1], hits[:h]

    def capped_seeds_device(self, d_patterns, d_offsets, n_patterns, min_length, max_length, max_count, hit_max, sample, d_seed_offsets,
                            d_seeds, seed_capacity, d_hit_offsets, d_hits, hit_capacity, stream=0):
        """gcsa2_capped_seeds_device on caller-owned device buffers (raw pointers): d_seed_offsets n_patterns + 1 u64, d_seeds
        seed_capacity records of five u64, d_hit_offsets seed_capacity + 1 entries, d_hits hit_capacity values.  `sample`: a
        bool, or the `over` policy as an int.  Complete on return.  Returns (seeds, hits); raises Gcsa2Error (BUFFER_TOO_SMALL,
        `.needed` = (seeds, hits)) when a buffer is too small."""
        total_m, total_h = C.c_uint64(), C.c_uint64()
        over = sample if isinstance(sample, int) and not isinstance(sample, bool) else (1 if sample else 0)
        rc = self._L.gcsa2_capped_seeds_device(self._h, d_patterns, d_offsets, n_patterns, int(min_length), int(max_length), int(max_count),
                                               int(hit_max), over, d_seed_offsets, d_seeds or None, int(seed_capacity), C.byref(total_m),
                                               d_hit_offsets, d_hits or None, int(hit_capacity), C.byref(total_h), stream)
        if rc != 0:
            err = Gcsa2Error(rc, self._L.gcsa2_last_error().decode(errors="replace"))
            err.needed = (total_m.value, total_h.value)
            raise err
        return total_m.value, total_h.value

    def kmer_support_batch(self, patterns, offsets, k, stride=1, hit_max=0, shift=11, n_bins=None, per_bin=False, support=None):
        """Read k-mers summed per graph node (gcsa2_kmer_support_batch): (support, stats).  Every window P_q[j stride, j stride +
        k) with a non-empty find() and hit_max == 0 or count() <= hit_max adds 1 to support[v >> shift] for every located value
        v of its range (per_bin: once per distinct bin); shift = 11 gives node ids, 0 exact positions.  Needs n_bins (a fresh
        zeroed array) or `support`, a uint64 array that is added into.  Contributions to bins >= n_bins are counted in
        stats["dropped"].  stats: a dict of SUPPORT_STATS."""
        patterns = np.ascontiguousarray(patterns, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = max(offsets.shape[0], 1) - 1
        if support is None:
            if n_bins is None:
                raise ValueError("kmer_support_batch needs n_bins or a support array to add into")
            support = np.zeros(int(n_bins), dtype=np.uint64)
        else:
            assert support.dtype == np.uint64 and support.ndim == 1 and support.flags.c_contiguous
            if n_bins is not None and int(n_bins) != support.shape[0]:
                raise ValueError("n_bins differs from the length of the support array")
        stats = (C.c_uint64 * len(SUPPORT_STATS))()
        _check(self._L.gcsa2_kmer_support_batch(self._h, _p8(patterns), _p64(offsets), n, int(k), int(stride), int(hit_max), int(shift),
                                                SUPPORT_PER_BIN if per_bin else 0, support.ctypes.data if support.shape[0] else None,
                                                support.shape[0], stats))
        return support, dict(zip(SUPPORT_STATS, (int(x) for x in stats)))

    def kmer_support_device(self, d_patterns, d_offsets, n_patterns, k, stride, hit_max, shift, flags, d_support, n_bins, stream=0):
        """gcsa2_kmer_support_device on caller-owned device buffers (raw pointers): d_support n_bins u64 that are added into
        (0 / None with n_bins == 0: a statistics run).  Complete on return.  Returns the stats as a dict of SUPPORT_STATS."""
        stats = (C.c_uint64 * len(SUPPORT_STATS))()
        rc = self._L.gcsa2_kmer_support_device(self._h, d_patterns, d_offsets, n_patterns, int(k), int(stride), int(hit_max), int(shift),
                                               int(flags), d_support or None, int(n_bins), stats, stream)
        if rc != 0:
            raise Gcsa2Error(rc, self._L.gcsa2_last_error().decode(errors="replace"))
        return dict(zip(SUPPORT_STATS, (int(x) for x in stats)))

    def seed_support_device(self, d_seeds, n_seeds, d_weights, hit_max, shift, flags, d_support, n_bins, stream=0):
        """gcsa2_seed_support_device on caller-owned device buffers (raw pointers): d_seeds n_seeds records of five u64 (only sp
        and ep are read), d_weights n_seeds u64 or 0 / None (1 each), d_support n_bins u64 that are added into.  Complete on
        return.  Returns the stats as a dict of SUPPORT_STATS."""
        stats = (C.c_uint64 * len(SUPPORT_STATS))()
        rc = self._L.gcsa2_seed_support_device(self._h, d_seeds or None, int(n_seeds), d_weights or None, int(hit_max), int(shift), int(flags),
                                               d_support or None, int(n_bins), stats, stream)
        if rc != 0:
            raise Gcsa2Error(rc, self._L.gcsa2_last_error().decode(errors="replace"))
        return dict(zip(SUPPORT_STATS, (int(x) for x in stats)))

    def kmer_spectrum(self, k, n_hist=4096, counts=True, include_Ns=False, force=False):
        """The occurrence histogram of the index's own k-mers (gcsa2_kmer_spectrum): (histogram, stats).  histogram[v] is the
        number of distinct k-mers whose value -- count(range) with counts, Range::length(range) without -- is v; the last of the
        n_hist bins collects everything at or above it (n_hist = 0: no histogram, an empty array).  stats: a dict of
        SPECTRUM_STATS; stats["kmers"] is count_kmers(k, include_Ns, force)."""
        histogram = np.zeros(int(n_hist), dtype=np.uint64)
        stats = (C.c_uint64 * len(SPECTRUM_STATS))()
        _check(self._L.gcsa2_kmer_spectrum(self._h, int(k), int(include_Ns), int(force), SPECTRUM_COUNTS if counts else 0,
                                           histogram.ctypes.data if histogram.shape[0] else None, histogram.shape[0], stats))
        return histogram, dict(zip(SPECTRUM_STATS, (int(x) for x in stats)))

    def list_kmers(self, k, min_value=0, max_value=0, counts=True, include_Ns=False, force=False):
        """The index's k-mers whose value lies in [min_value, max_value] (max_value = 0: no upper end), as an (m, 8) uint64 array
        with the columns INDEX_KMER (gcsa2_list_kmers): a sizing call, then a filling call.  Order is unspecified; the key is
        packed as in compare_kmers_records; `count` is 0 without counts."""
        flags = SPECTRUM_COUNTS if counts else 0
        total = C.c_uint64(0)
        rc = self._L.gcsa2_list_kmers(self._h, int(k), int(include_Ns), int(force), flags, int(min_value), int(max_value), None, 0, C.byref(total))
        if rc != STATUS_BUFFER_TOO_SMALL:
            _check(rc)
        records = np.zeros((total.value, 8), dtype=np.uint64)
        if total.value:
            _check(self._L.gcsa2_list_kmers(self._h, int(k), int(include_Ns), int(force), flags, int(min_value), int(max_value),
                                            records.ctypes.data, total.value, C.byref(total)))
        return records[: total.value]

    def index_kmer_support_device(self, k, hit_max, shift, flags, d_support, n_bins, include_Ns=False, force=False, stream=0):
        """gcsa2_index_kmer_support_device: every k-mer of the index with hit_max == 0 or count() <= hit_max adds 1 to
        d_support[v >> shift] for every located value v of its range (SUPPORT_PER_BIN: once per distinct bin).  d_support: a raw
        device pointer to n_bins u64 that are added into (0 / None with n_bins == 0: a statistics run).  Complete on return.
        Returns the stats as a dict of SUPPORT_STATS."""
        stats = (C.c_uint64 * len(SUPPORT_STATS))()
        rc = self._L.gcsa2_index_kmer_support_device(self._h, int(k), int(include_Ns), int(force), int(hit_max), int(shift), int(flags),
                                                     d_support or None, int(n_bins), stats, stream)
        if rc != 0:
            raise Gcsa2Error(rc, self._L.gcsa2_last_error().decode(errors="replace"))
        return dict(zip(SUPPORT_STATS, (int(x) for x in stats)))

    def index_kmer_support(self, k, n_bins, hit_max=0, shift=11, per_bin=False, include_Ns=False, force=False):
        """The host convenience of index_kmer_support_device: (support, stats) with a fresh array of n_bins, through a zeroed
        device array of the index's device (torch is the plumbing)."""
        import torch
        d = torch.zeros(max(int(n_bins), 1), dtype=torch.int64, device=torch.device("cuda", int(self._L.gcsa2_device(self._h))))
        stats = self.index_kmer_support_device(k, hit_max, shift, SUPPORT_PER_BIN if per_bin else 0, d.data_ptr() if n_bins else 0, n_bins,
                                               include_Ns=include_Ns, force=force)
        return d[: int(n_bins)].cpu().numpy().view(np.uint64), stats

    def kmer_classes_batch(self, patterns, offsets, k, class_of_bin, n_classes, stride=1, hit_max=0, shift=11, per_window=False,
                           unambiguous=False, votes=True, calls=True):
        """Per read, the votes of its k-mers over classes of graph nodes (gcsa2_kmer_classes_batch): (votes, calls, stats).
        Every window P_q[j stride, j stride + k) with a non-empty find() and hit_max == 0 or count() <= hit_max votes for the
        class class_of_bin[v >> shift] of every located value v of its range (a uint32 array; CLASS_NONE, an id >= n_classes
        or a bin beyond the array: no class): n_c votes for class c, once per class with per_window, and only when all its
        values share one class with unambiguous.  votes: (reads, n_classes) uint64, written, not added to; calls: (reads, 6)
        uint64 with the columns CLASS_CALL; either is None when not asked for.  stats: a dict of CLASS_STATS."""
        patterns = np.ascontiguousarray(patterns, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        class_of_bin = np.ascontiguousarray(class_of_bin, dtype=np.uint32)
        n = max(offsets.shape[0], 1) - 1
        out_votes = np.zeros((n, int(n_classes)), dtype=np.uint64) if votes else None
        out_calls = np.zeros((n, len(CLASS_CALL)), dtype=np.uint64) if calls else None
        stats = (C.c_uint64 * len(CLASS_STATS))()
        flags = (CLASS_PER_WINDOW if per_window else 0) | (CLASS_UNAMBIGUOUS if unambiguous else 0)
        _check(self._L.gcsa2_kmer_classes_batch(self._h, _p8(patterns), _p64(offsets), n, int(k), int(stride), int(hit_max), int(shift), flags,
                                                class_of_bin.ctypes.data if class_of_bin.shape[0] else None, class_of_bin.shape[0], int(n_classes),
                                                out_votes.ctypes.data if votes else None, out_calls.ctypes.data if calls else None, stats))
        return out_votes, out_calls, dict(zip(CLASS_STATS, (int(x) for x in stats)))

    def kmer_classes_device(self, d_patterns, d_offsets, n_patterns, k, stride, hit_max, shift, flags, d_class_of_bin, n_bins, n_classes,
                            d_votes, d_calls, stream=0, want_stats=True):
        """gcsa2_kmer_classes_device on caller-owned device buffers (raw pointers): d_class_of_bin n_bins u32, d_votes n_patterns x
        n_classes u64 and d_calls n_patterns records of six u64, both written (0 / None: not wanted).  Complete on return.
        Returns the stats as a dict of CLASS_STATS, or None with want_stats=False (a NULL stats pointer)."""
        stats = (C.c_uint64 * len(CLASS_STATS))() if want_stats else None
        rc = self._L.gcsa2_kmer_classes_device(self._h, d_patterns, d_offsets, n_patterns, int(k), int(stride), int(hit_max), int(shift), int(flags),
                                               d_class_of_bin or None, int(n_bins), int(n_classes), d_votes or None, d_calls or None, stats, stream)
        if rc != 0:
            raise Gcsa2Error(rc, self._L.gcsa2_last_error().decode(errors="replace"))
        return dict(zip(CLASS_STATS, (int(x) for x in stats))) if want_stats else None

    def seed_classes_device(self, d_group_offsets, n_groups, d_seeds, n_seeds, d_weights, hit_max, shift, flags, d_class_of_bin, n_bins,
                            n_classes, d_votes, d_calls, stream=0, want_stats=True):
        """gcsa2_seed_classes_device on caller-owned device buffers (raw pointers): group g owns the records
        [d_group_offsets[g], d_group_offsets[g + 1]) of d_seeds (five u64 each, only sp and ep are read), d_weights n_seeds u64 or
        0 / None (1 each); the outputs as kmer_classes_device.  Complete on return.  Returns the stats or None."""
        stats = (C.c_uint64 * len(CLASS_STATS))() if want_stats else None
        rc = self._L.gcsa2_seed_classes_device(self._h, d_group_offsets or None, int(n_groups), d_seeds or None, int(n_seeds), d_weights or None,
                                               int(hit_max), int(shift), int(flags), d_class_of_bin or None, int(n_bins), int(n_classes),
                                               d_votes or None, d_calls or None, stats, stream)
        if rc != 0:
            raise Gcsa2Error(rc, self._L.gcsa2_last_error().decode(errors="replace"))
        return dict(zip(CLASS_STATS, (int(x) for x in stats))) if want_stats else None

    def kmer_top_classes_batch(self, patterns, offsets, k, class_of_bin, n_classes, top_n, stride=1, hit_max=0, shift=11, per_window=False,
                               unambiguous=False, top=True, summaries=True):
        """Per read, the top_n classes with the most votes of its k-mers (gcsa2_kmer_top_classes_batch): (top, summaries, stats).
        The votes are those of kmer_classes_batch, but n_classes may be up to 0xFFFFFFFF and no matrix exists.  top: (reads, top_n)
        of CLASS_VOTE, more votes first and the lower id on a tie, {UNKNOWN, 0} behind the voted classes; summaries: (reads,) of
        TOP_SUMMARY; either is None when not asked for.  stats: a dict of CLASS_STATS."""
        patterns = np.ascontiguousarray(patterns, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        class_of_bin = np.ascontiguousarray(class_of_bin, dtype=np.uint32)
        n = max(offsets.shape[0], 1) - 1
        out_top = np.zeros((n, max(int(top_n), 0)), dtype=CLASS_VOTE) if top else None
        out_sums = np.zeros(n, dtype=TOP_SUMMARY) if summaries else None
        stats = (C.c_uint64 * len(CLASS_STATS))()
        flags = (CLASS_PER_WINDOW if per_window else 0) | (CLASS_UNAMBIGUOUS if unambiguous else 0)
        _check(self._L.gcsa2_kmer_top_classes_batch(self._h, _p8(patterns), _p64(offsets), n, int(k), int(stride), int(hit_max), int(shift), flags,
                                                    class_of_bin.ctypes.data if class_of_bin.shape[0] else None, class_of_bin.shape[0], int(n_classes),
                                                    int(top_n), out_top.ctypes.data if top else None, out_sums.ctypes.data if summaries else None, stats))
        return out_top, out_sums, dict(zip(CLASS_STATS, (int(x) for x in stats)))

    def kmer_top_classes_device(self, d_patterns, d_offsets, n_patterns, k, stride, hit_max, shift, flags, d_class_of_bin, n_bins, n_classes,
                                top_n, d_top, d_summaries, stream=0, want_stats=True):
        """gcsa2_kmer_top_classes_device on caller-owned device buffers (raw pointers): d_class_of_bin n_bins u32, d_top n_patterns x
        top_n records of two u64 and d_summaries n_patterns records of three u64, both written (0 / None: not wanted).  Complete
        on return.  Returns the stats as a dict of CLASS_STATS, or None with want_stats=False (a NULL stats pointer)."""
        stats = (C.c_uint64 * len(CLASS_STATS))() if want_stats else None
        rc = self._L.gcsa2_kmer_top_classes_device(self._h, d_patterns, d_offsets, n_patterns, int(k), int(stride), int(hit_max), int(shift), int(flags),
                                                   d_class_of_bin or None, int(n_bins), int(n_classes), int(top_n), d_top or None, d_summaries or None,
                                                   stats, stream)
        if rc != 0:
            raise Gcsa2Error(rc, self._L.gcsa2_last_error().decode(errors="replace"))
        return dict(zip(CLASS_STATS, (int(x) for x in stats))) if want_stats else None

    def seed_top_classes_device(self, d_group_offsets, n_groups, d_seeds, n_seeds, d_weights, hit_max, shift, flags, d_class_of_bin, n_bins,
                                n_classes, top_n, d_top, d_summaries, stream=0, want_stats=True):
        """gcsa2_seed_top_classes_device on caller-owned device buffers (raw pointers): groups, records and weights as
        seed_classes_device, the outputs as kmer_top_classes_device.  Complete on return.  Returns the stats or None."""
        stats = (C.c_uint64 * len(CLASS_STATS))() if want_stats else None
        rc = self._L.gcsa2_seed_top_classes_device(self._h, d_group_offsets or None, int(n_groups), d_seeds or None, int(n_seeds), d_weights or None,
                                                   int(hit_max), int(shift), int(flags), d_class_of_bin or None, int(n_bins), int(n_classes),
                                                   int(top_n), d_top or None, d_summaries or None, stats, stream)
        if rc != 0:
            raise Gcsa2Error(rc, self._L.gcsa2_last_error().decode(errors="replace"))
        return dict(zip(CLASS_STATS, (int(x) for x in stats))) if want_stats else None

    def _clusters_done(self, rc, stats, want_stats):
        if rc != 0:
            raise Gcsa2Error(rc, self._L.gcsa2_last_error().decode(errors="replace"))
        return dict(zip(CLUSTER_STATS, (int(x) for x in stats))) if want_stats else None

    def seed_clusters_device(self, d_group_offsets, n_groups, d_seeds, n_seeds, d_hit_offsets, d_hits, n_hits, shift, d_coord_of_bin, n_bins,
                             band, top_n, d_top, d_summaries, stream=0, want_stats=True):
        """gcsa2_seed_clusters_device on caller-owned device buffers (raw pointers): a seed CSR with its hit offsets and hits as any
        hits call emits them, d_coord_of_bin n_bins u64, d_top n_groups x top_n records of eight u64 (CLUSTER) and d_summaries
        n_groups records of three u64 (CLUSTER_SUMMARY), both written (0 / None: not wanted).  Complete on return.  Returns the
        stats as a dict of CLUSTER_STATS, or None with want_stats=False (a NULL stats pointer)."""
        stats = (C.c_uint64 * len(CLUSTER_STATS))() if want_stats else None
        rc = self._L.gcsa2_seed_clusters_device(self._h, d_group_offsets or None, int(n_groups), d_seeds or None, int(n_seeds), d_hit_offsets or None,
                                                d_hits or None, int(n_hits), int(shift), d_coord_of_bin or None, int(n_bins), int(band), int(top_n),
                                                d_top or None, d_summaries or None, stats, stream)
        return self._clusters_done(rc, stats, want_stats)

    def kmer_clusters_device(self, d_patterns, d_offsets, n_patterns, k, stride, hit_max, sample, shift, d_coord_of_bin, n_bins, band, top_n,
                             d_top, d_summaries, stream=0, want_stats=True):
        """gcsa2_kmer_clusters_device: kmer_hits_device and seed_clusters_device in one call, the hits staying on the device."""
        stats = (C.c_uint64 * len(CLUSTER_STATS))() if want_stats else None
        over = sample if isinstance(sample, int) and not isinstance(sample, bool) else (1 if sample else 0)
        rc = self._L.gcsa2_kmer_clusters_device(self._h, d_patterns, d_offsets, n_patterns, int(k), int(stride), int(hit_max), over,
                                                int(shift), d_coord_of_bin or None, int(n_bins), int(band), int(top_n), d_top or None, d_summaries or None,
                                                stats, stream)
        return self._clusters_done(rc, stats, want_stats)

    def minimizer_clusters_device(self, d_patterns, d_offsets, n_patterns, k, w, hash_seed, hit_max, sample, shift, d_coord_of_bin, n_bins, band,
                                  top_n, d_top, d_summaries, stream=0, want_stats=True):
        """gcsa2_minimizer_clusters_device: minimizer_hits_device and seed_clusters_device in one call."""
        stats = (C.c_uint64 * len(CLUSTER_STATS))() if want_stats else None
        over = sample if isinstance(sample, int) and not isinstance(sample, bool) else (1 if sample else 0)
        rc = self._L.gcsa2_minimizer_clusters_device(self._h, d_patterns, d_offsets, n_patterns, int(k), int(w), int(hash_seed), int(hit_max), over,
                                                     int(shift), d_coord_of_bin or None, int(n_bins), int(band), int(top_n), d_top or None,
                                                     d_summaries or None, stats, stream)
        return self._clusters_done(rc, stats, want_stats)

    def _clusters_batch(self, call, patterns, offsets, head, hit_max, sample, shift, coord_of_bin, band, top_n, top, summaries):
        patterns = np.ascontiguousarray(patterns, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        coord_of_bin = np.ascontiguousarray(coord_of_bin, dtype=np.uint64)
        n = max(offsets.shape[0], 1) - 1
        out_top = np.zeros((n, max(int(top_n), 0), len(CLUSTER)), dtype=np.uint64) if top else None
        out_sums = np.zeros((n, len(CLUSTER_SUMMARY)), dtype=np.uint64) if summaries else None
        stats = (C.c_uint64 * len(CLUSTER_STATS))()
        over = sample if isinstance(sample, int) and not isinstance(sample, bool) else (1 if sample else 0)
        _check(call(self._h, _p8(patterns), _p64(offsets), n, *head, int(hit_max), over, int(shift),
                    coord_of_bin.ctypes.data if coord_of_bin.shape[0] else None, coord_of_bin.shape[0], int(band), int(top_n),
                    out_top.ctypes.data if top else None, out_sums.ctypes.data if summaries else None, stats))
        return out_top, out_sums, dict(zip(CLUSTER_STATS, (int(x) for x in stats)))

    def kmer_clusters_batch(self, patterns, offsets, k, coord_of_bin, top_n, stride=1, hit_max=0, sample=False, shift=10, band=0, top=True,
                            summaries=True):
        """Per read, the top_n diagonal bands of the hits of its k-mers (gcsa2_kmer_clusters_batch): (top, summaries, stats).  top:
        (reads, top_n, 8) uint64 with the columns CLUSTER, larger covered first, all zero behind the last cluster; summaries:
        (reads, 3) uint64 with the columns CLUSTER_SUMMARY; either is None when not asked for.  stats: a dict of CLUSTER_STATS.
        coord_of_bin: uint64 coordinates of the bins value >> shift, UNKNOWN for a bin without one."""
        return self._clusters_batch(self._L.gcsa2_kmer_clusters_batch, patterns, offsets, (int(k), int(stride)), hit_max, sample, shift, coord_of_bin,
                                    band, top_n, top, summaries)

    def minimizer_clusters_batch(self, patterns, offsets, k, w, coord_of_bin, top_n, hash_seed=0, hit_max=0, sample=False, shift=10, band=0,
                                 top=True, summaries=True):
        """The same over the (w, k)-minimizers of every read (gcsa2_minimizer_clusters_batch)."""
        return self._clusters_batch(self._L.gcsa2_minimizer_clusters_batch, patterns, offsets, (int(k), int(w), int(hash_seed)), hit_max, sample,
                                    shift, coord_of_bin, band, top_n, top, summaries)

    def lf_node_batch(self, nodes):
        nodes = np.ascontiguousarray(nodes, dtype=np.uint64)
        out = np.zeros_like(nodes)
        _check(self._L.gcsa2_lf_node_batch(self._h, _p64(nodes), nodes.shape[0], _p64(out)))
        return out

    def LF(self, arg, comp=None):
        if comp is None:
            return int(self.lf_node_batch(np.array([arg], dtype=np.uint64))[0])
        r = self.lf_batch(np.array([arg], dtype=np.uint64), np.array([comp], dtype=np.uint8))[0]
        return (int(r[0]), int(r[1]))

    def charRange(self, comp):
        sp, ep = C.c_uint64(), C.c_uint64()
        _check(self._L.gcsa2_char_range(self._h, comp, C.byref(sp), C.byref(ep)))
        return (sp.value, ep.value)

    def lf_all_batch(self, ranges, all_comps):
        ranges = _ranges(ranges)
        out = np.zeros((ranges.shape[0], self.sigma, 2), dtype=np.uint64)
        _check(self._L.gcsa2_lf_all_batch(self._h, _p64(ranges), ranges.shape[0], int(all_comps), _p64(out)))
        return out

    def LF_fast(self, rng):
        return [(int(a), int(b)) for a, b in self.lf_all_batch(np.array([rng], dtype=np.uint64), 0)[0]]

    def LF_all(self, rng):
        return [(int(a), int(b)) for a, b in self.lf_all_batch(np.array([rng], dtype=np.uint64), 1)[0]]

    # ---- count --------------------------------------------------------------------------
    def count_batch(self, ranges):
        ranges = _ranges(ranges)
        out = np.zeros(ranges.shape[0], dtype=np.uint64)
        _check(self._L.gcsa2_count_batch(self._h, _p64(ranges), ranges.shape[0], _p64(out)))
        return out

    def count(self, rng):
        return int(self.count_batch(np.array([rng], dtype=np.uint64))[0])

    # ---- locate -------------------------------------------------------------------------
    def locate_batch(self, ranges, sort=True):
        """CSR (offsets[nq+1], values): sorted distinct node_type values per range
        (sort=False: path order with duplicates, as the reference's sort == false)."""
        ranges = _ranges(ranges)
        nq = ranges.shape[0]
        offsets = np.zeros(nq + 1, dtype=np.uint64)
        job = C.c_void_p()
        _check(self._L.gcsa2_locate_run(self._h, _p64(ranges), nq, int(sort), _p64(offsets), C.byref(job)))
        values = np.zeros(max(int(offsets[nq]), 1), dtype=np.uint64)
        _check(self._L.gcsa2_locate_fetch(job, _p64(values), values.shape[0]))
        return offsets, values[: int(offsets[nq])]

    def locate(self, rng, sort=True, max_positions=None):
        """locate(path_node) / locate(range) / locate(range, max_positions) (gcsa.h:126-128)."""
        if isinstance(rng, (int, np.integer)):
            rng = (int(rng), int(rng))
        if max_positions is None:
            return self.locate_batch(np.array([rng], dtype=np.uint64), sort)[1]
        cap = max(1, min(int(max_positions), self.count(rng)))
        values = np.zeros(cap, dtype=np.uint64)
        cnt = C.c_uint64()
        _check(self._L.gcsa2_locate_max(self._h, rng[0], rng[1], max_positions, _p64(values), cap, C.byref(cnt)))
        return values[: cnt.value]

    def locate_max_batch(self, ranges, max_positions):
        """locate(range, max_positions) for every range (gcsa2_locate_max_batch): CSR (offsets[nq+1], values), where
        offsets[q+1] - offsets[q] = min(max_positions, count(range q)) and each range's values are those of `locate`."""
        ranges = _ranges(ranges)
        nq = ranges.shape[0]
        mx = int(max_positions)
        # room for min(max_positions, count) per range, in Python integers; a count() that wrapped below zero says nothing
        # of the range's size, so the call is repeated with the size it asks for when this is not enough
        cap = sum(min(mx, int(c)) for c in self.count_batch(ranges) if int(c) < (1 << 40)) if nq else 0
        offsets = np.zeros(nq + 1, dtype=np.uint64)
        total = C.c_uint64()
        for _ in range(2):
            values = np.zeros(max(cap, 1), dtype=np.uint64)
            rc = self._L.gcsa2_locate_max_batch(self._h, _p64(ranges), nq, mx, _p64(offsets), _p64(values), cap, C.byref(total))
            if rc != STATUS_BUFFER_TOO_SMALL or total.value <= cap:
                break
            cap = total.value
        _check(rc)
        return offsets, values[: total.value]

    def compare_kmers(self, other, k, include_Ns=False, force=False):
        """`compareKMers(self, other, k)` (reference src/algorithms.cpp:534-616): (shared, left, right)."""
        out = np.zeros(3, dtype=np.uint64)
        _check(self._L.gcsa2_compare_kmers(self._h, other._h, k, int(include_Ns), int(force), _p64(out)))
        return tuple(int(x) for x in out)

    def compare_kmers_records(self, other, k, include_Ns=False, force=False):
        """compareKMers with parameters.output: (counts, left_states, right_states), states as
        (count, 8) uint64 arrays in the layout of the reference's .left / .right dumps."""
        counts = self.compare_kmers(other, k, include_Ns, force)
        left = np.zeros((max(counts[1], 1), 8), dtype=np.uint64)
        right = np.zeros((max(counts[2], 1), 8), dtype=np.uint64)
        out = np.zeros(3, dtype=np.uint64)
        _check(self._L.gcsa2_compare_kmers_records(self._h, other._h, k, int(include_Ns), int(force), _p64(out),
                                                   _p64(left), counts[1], _p64(right), counts[2]))
        return tuple(int(x) for x in out), left[: counts[1]], right[: counts[2]]

    def match_stats_batch(self, patterns, offsets, out=None):
        """Matching statistics by fused LF + parent (needs the LCP array):
        (ms uint16[total bytes], ranges (nq, 2), parent() calls per pattern).  `out`: the three arrays of an earlier call
        of the same shape, to be filled again (fresh arrays cost their page faults: 0.5 GB for 1 M x 256 bp)."""
        patterns = np.ascontiguousarray(patterns, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        nq = offsets.shape[0] - 1
        if out is not None:
            ms, ranges, fallbacks = out
            if isinstance(ms.base, np.ndarray) and ms.base.dtype == np.uint16 and ms.base.ndim == 1 and ms.base.shape[0] >= max(int(offsets[nq]), 1):
                ms = ms.base              # the slice an earlier call returned: its whole array
            assert ms.dtype == np.uint16 and ms.shape[0] >= int(offsets[nq]) and ranges.shape == (nq, 2) and fallbacks.shape == (nq,)
        else:
            ms = np.zeros(max(int(offsets[nq]), 1), dtype=np.uint16)
            ranges = np.zeros((nq, 2), dtype=np.uint64)
            fallbacks = np.zeros(nq, dtype=np.uint64)
        _check(self._L.gcsa2_match_stats_batch(self._h, _p8(patterns), _p64(offsets), nq, ms.ctypes.data,
                                               _p64(ranges), _p64(fallbacks)))
        return ms[: int(offsets[nq])], ranges, fallbacks

    def match_stats_device(self, d_patterns, d_offsets, nq, d_ms, d_ranges, d_fallbacks=0, stream=0, variant=0, total_bytes=None):
        """total_bytes = offsets[nq] when the caller knows it: the call then only enqueues (otherwise it reads that
        value back from the device, which waits for the stream once)."""
        if total_bytes is None:
            _check(self._L.gcsa2_match_stats_device_variant(self._h, variant, d_patterns, d_offsets, nq, d_ms, d_ranges, d_fallbacks, stream))
        else:
            _check(self._L.gcsa2_match_stats_device_sized(self._h, variant, d_patterns, d_offsets, nq, int(total_bytes), d_ms, d_ranges,
                                                          d_fallbacks, stream))

    def match_breaks_batch(self, patterns, offsets, min_length=0, capacity=None, out=None, max_length=0):
        """Break points of a batch in host memory: (break_offsets (nq + 1), breaks (total, 4) = {position, length, sp, ep}, ranges,
        parent() counts).  The record buffer is sized from the refusal when `capacity` is too small (default: 4 per pattern).
        `out` = (break_offsets, breaks, ranges, fallbacks) arrays of the caller (a caller that reuses them avoids the page faults
        of fresh ones); too few rows in `breaks` raise BUFFER_TOO_SMALL with `needed`.  max_length > 0: no match grows beyond
        that many characters (gcsa2_match_breaks_bounded_batch; a mapper passes order()); 0: no cap."""
        patterns = np.ascontiguousarray(patterns, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        nq = offsets.shape[0] - 1
        if out is not None:
            boff, brk, rng, fb = out
            assert boff.dtype == np.uint64 and boff.shape[0] >= nq + 1 and brk.dtype == np.uint64 and brk.flags.c_contiguous and brk.shape[1] == 4
            assert rng.dtype == np.uint64 and rng.shape[0] >= nq and fb.dtype == np.uint64 and fb.shape[0] >= nq
            total = C.c_uint64()
            rc = self._L.gcsa2_match_breaks_bounded_batch(self._h, _p8(patterns), _p64(offsets), nq, int(min_length), int(max_length), _p64(boff), brk.ctypes.data, brk.shape[0],
                                                  C.byref(total), rng.ctypes.data, fb.ctypes.data)
            if rc == -6:
                err = Gcsa2Error(rc, self._L.gcsa2_last_error().decode(errors="replace"))
                err.needed = total.value
                raise err
            _check(rc)
            return boff[: nq + 1], brk[: total.value], rng[:nq], fb[:nq]
        cap = int(capacity if capacity is not None else 4 * nq + 16)
        boff = np.zeros(nq + 1, dtype=np.uint64)
        rng = np.zeros((max(nq, 1), 2), dtype=np.uint64)
        fb = np.zeros(max(nq, 1), dtype=np.uint64)
        total = C.c_uint64()
        for _ in range(2):
            brk = np.zeros((max(cap, 1), 4), dtype=np.uint64)
            rc = self._L.gcsa2_match_breaks_bounded_batch(self._h, _p8(patterns), _p64(offsets), nq, int(min_length), int(max_length), _p64(boff), brk.ctypes.data, cap,
                                                  C.byref(total), rng.ctypes.data, fb.ctypes.data)
            if rc == -6 and total.value > cap:
                cap = total.value
                continue
            _check(rc)
            return boff, brk[: total.value], rng[:nq], fb[:nq]
        _check(rc)

    def match_breaks_device(self, d_patterns, d_offsets, nq, total_bytes, d_break_offsets, d_breaks, capacity, d_ranges=0, d_fallbacks=0,
                            stream=0, variant=0, min_length=0, max_length=0):
        """Matching statistics as break points (gcsa2_match_breaks_device): the CSR of the left-maximal matches, records of four
        u64 {position, length, sp, ep}; returns the number of records.  Raises Gcsa2Error (BUFFER_TOO_SMALL, `.needed`) when
        `capacity` records are not enough.  max_length > 0 caps the matches (gcsa2_match_breaks_bounded_device)."""
        total = C.c_uint64()
        tb = 0xFFFFFFFFFFFFFFFF if total_bytes is None else int(total_bytes)
        rc = self._L.gcsa2_match_breaks_bounded_device(self._h, d_patterns, d_offsets, nq, tb, variant, int(min_length), int(max_length), d_break_offsets, d_breaks, capacity, C.byref(total),
                                               d_ranges, d_fallbacks, stream)
        if rc != 0:
            err = Gcsa2Error(rc, self._L.gcsa2_last_error().decode(errors="replace"))
            err.needed = total.value
            raise err
        return total.value

    def mem_hits_batch(self, patterns, offsets, min_length, hit_max=0, sample=False, out=None, max_length=0):
        """MEM hits of a batch in host memory (gcsa2_mem_hits_batch): (mem_offsets (nq + 1), mems (total, 5) = {position, length,
        sp, ep, count}, hit_offsets (total + 1), hits).  A MEM's hits are its locate() values when hit_max == 0 or its count is at
        most hit_max; above the cap none (sample=False) or locate(range, hit_max) (sample=True).  The buffers are grown from the
        refusal.  `out` = (mem_offsets, mems, hit_offsets, hits) arrays of the caller; too small ones raise BUFFER_TOO_SMALL with
        `needed` = (MEMs, hits).  max_length > 0: the MEMs of match_breaks_batch(max_length=...) (gcsa2_mem_hits_bounded_batch)."""
        patterns = np.ascontiguousarray(patterns, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        nq = offsets.shape[0] - 1
        over = 1 if sample else 0
        total_m, total_h = C.c_uint64(), C.c_uint64()

        def call(moff, mems, hoff, hits):
            assert moff.dtype == np.uint64 and moff.shape[0] >= nq + 1 and mems.dtype == np.uint64 and mems.flags.c_contiguous
            assert mems.shape[1] == 5 and hoff.dtype == np.uint64 and hoff.shape[0] >= mems.shape[0] + 1 and hits.dtype == np.uint64
            return self._L.gcsa2_mem_hits_bounded_batch(self._h, _p8(patterns), _p64(offsets), nq, int(min_length), int(max_length), int(hit_max), over,
                                                moff.ctypes.data, mems.ctypes.data, mems.shape[0], C.byref(total_m),
                                                hoff.ctypes.data, hits.ctypes.data, hits.shape[0], C.byref(total_h))

        if out is not None:
            moff, mems, hoff, hits = out
            rc = call(moff, mems, hoff, hits)
        else:
            mcap, hcap = 4 * nq + 16, 16 * nq + 64
            moff = np.zeros(nq + 1, dtype=np.uint64)
            for _ in range(2):
                mems = np.zeros((mcap, 5), dtype=np.uint64)
                hoff = np.zeros(mcap + 1, dtype=np.uint64)
                hits = np.zeros(hcap, dtype=np.uint64)
                rc = call(moff, mems, hoff, hits)
                if rc != STATUS_BUFFER_TOO_SMALL:
                    break
                mcap, hcap = max(mcap, total_m.value), max(hcap, total_h.value)
        if rc == STATUS_BUFFER_TOO_SMALL:
            err = Gcsa2Error(rc, self._L.gcsa2_last_error().decode(errors="replace"))
            err.needed = (total_m.value, total_h.value)
            raise err
        _check(rc)
        m, h = total_m.value, total_h.value
        return moff[: nq + 1], mems[:m], hoff[: m + 1], hits[:h]

    def mem_hits_device(self, d_patterns, d_offsets, nq, total_bytes, min_length, hit_max, sample, d_mem_offsets, d_mems, mem_capacity,
                        d_hit_offsets, d_hits, hit_capacity, stream=0, max_length=0):
        """MEM hits into caller-owned device buffers (gcsa2_mem_hits_device): d_mems holds mem_capacity records of five u64,
        d_hit_offsets mem_capacity + 1 entries, d_hits hit_capacity values; total_bytes None = read back.  Returns (MEMs, hits);
        raises Gcsa2Error (BUFFER_TOO_SMALL, `.needed` = (MEMs, hits)) when a buffer is too small.  max_length > 0 caps the
        matches (gcsa2_mem_hits_bounded_device)."""
        total_m, total_h = C.c_uint64(), C.c_uint64()
        tb = 0xFFFFFFFFFFFFFFFF if total_bytes is None else int(total_bytes)
        over = sample if isinstance(sample, int) and not isinstance(sample, bool) else (1 if sample else 0)
        rc = self._L.gcsa2_mem_hits_bounded_device(self._h, d_patterns, d_offsets, nq, tb, int(min_length), int(max_length), int(hit_max), over, d_mem_offsets,
                                           d_mems, mem_capacity, C.byref(total_m), d_hit_offsets, d_hits, hit_capacity, C.byref(total_h),
                                           stream)
        if rc != 0:
            err = Gcsa2Error(rc, self._L.gcsa2_last_error().decode(errors="replace"))
            err.needed = (total_m.value, total_h.value)
            raise err
        return total_m.value, total_h.value

    def sub_mem_hits_batch(self, patterns, offsets, mem_offsets, mems, min_length, reseed_length, hit_max=0, sample=False, out=None):
        """Sub-MEM reseeding of a batch in host memory (gcsa2_sub_mem_hits_batch): inside every MEM (rows of `mems`, five u64
        {position, length, sp, ep, count} as mem_hits_batch returns them, per pattern by `mem_offsets`) of at least
        reseed_length bases, the matches of at least min_length that occur more often than the MEM.  Returns (sub_offsets
        (MEMs + 1), subs (total, 5), hit_offsets (total + 1), hits); hits follow mem_hits_batch's rules.  The buffers are grown
        from the refusal.  `out` = (sub_offsets, subs, hit_offsets, hits) arrays of the caller; too small ones raise
        BUFFER_TOO_SMALL with `needed` = (sub-MEMs, hits)."""
        patterns = np.ascontiguousarray(patterns, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        mem_offsets = np.ascontiguousarray(mem_offsets, dtype=np.uint64)
        mems = np.ascontiguousarray(mems, dtype=np.uint64).reshape(-1, 5)
        nq, nm = offsets.shape[0] - 1, mems.shape[0]
        over = 1 if sample else 0
        total_s, total_h = C.c_uint64(), C.c_uint64()

        def call(soff, subs, hoff, hits):
            assert soff.dtype == np.uint64 and soff.shape[0] >= nm + 1 and subs.dtype == np.uint64 and subs.flags.c_contiguous
            assert subs.shape[1] == 5 and hoff.dtype == np.uint64 and hoff.shape[0] >= subs.shape[0] + 1 and hits.dtype == np.uint64
            return self._L.gcsa2_sub_mem_hits_batch(self._h, _p8(patterns), _p64(offsets), nq, _p64(mem_offsets), mems.ctypes.data, nm,
                                                    int(min_length), int(reseed_length), int(hit_max), over, soff.ctypes.data, subs.ctypes.data,
                                                    subs.shape[0], C.byref(total_s), hoff.ctypes.data, hits.ctypes.data, hits.shape[0],
                                                    C.byref(total_h))

        if out is not None:
            soff, subs, hoff, hits = out
            rc = call(soff, subs, hoff, hits)
        else:
            scap, hcap = 4 * nm + 16, 16 * nm + 64
            soff = np.zeros(nm + 1, dtype=np.uint64)
            for _ in range(2):
                subs = np.zeros((scap, 5), dtype=np.uint64)
                hoff = np.zeros(scap + 1, dtype=np.uint64)
                hits = np.zeros(hcap, dtype=np.uint64)
                rc = call(soff, subs, hoff, hits)
                if rc != STATUS_BUFFER_TOO_SMALL:
                    break
                scap, hcap = max(scap, total_s.value), max(hcap, total_h.value)
        if rc == STATUS_BUFFER_TOO_SMALL:
            err = Gcsa2Error(rc, self._L.gcsa2_last_error().decode(errors="replace"))
            err.needed = (total_s.value, total_h.value)
            raise err
        _check(rc)
        s, h = total_s.value, total_h.value
        return soff[: nm + 1], subs[:s], hoff[: s + 1], hits[:h]

    def sub_mem_hits_device(self, d_patterns, d_offsets, nq, total_bytes, d_mem_offsets, d_mems, n_mems, min_length, reseed_length, hit_max,
                            sample, d_sub_offsets, d_subs, sub_capacity, d_hit_offsets, d_hits, hit_capacity, stream=0):
        """Sub-MEM reseeding into caller-owned device buffers (gcsa2_sub_mem_hits_device): d_mems holds n_mems records of five
        u64 (None = read d_mem_offsets[nq]), d_sub_offsets n_mems + 1 entries, d_subs sub_capacity records, d_hit_offsets
        sub_capacity + 1 entries, d_hits hit_capacity values.  Returns (sub-MEMs, hits); raises Gcsa2Error (BUFFER_TOO_SMALL,
        `.needed` = (sub-MEMs, hits)) when a buffer is too small."""
        total_s, total_h = C.c_uint64(), C.c_uint64()
        tb = 0xFFFFFFFFFFFFFFFF if total_bytes is None else int(total_bytes)
        nm = 0xFFFFFFFFFFFFFFFF if n_mems is None else int(n_mems)
        over = sample if isinstance(sample, int) and not isinstance(sample, bool) else (1 if sample else 0)
        rc = self._L.gcsa2_sub_mem_hits_device(self._h, d_patterns, d_offsets, nq, tb, d_mem_offsets, d_mems, nm, int(min_length),
                                               int(reseed_length), int(hit_max), over, d_sub_offsets, d_subs, sub_capacity, C.byref(total_s),
                                               d_hit_offsets, d_hits, hit_capacity, C.byref(total_h), stream)
        if rc != 0:
            err = Gcsa2Error(rc, self._L.gcsa2_last_error().decode(errors="replace"))
            err.needed = (total_s.value, total_h.value)
            raise err
        return total_s.value, total_h.value

    def match_stats_profile_device(self, d_patterns, d_offsets, nq, total_bytes, d_ms, d_ranges, d_fallbacks, d_prof, stream=0):
        """Diagnostic: the instrumented matching-statistics kernel (cycles per phase and event counts into d_prof[16])."""
        _check(self._L.gcsa2_match_stats_profile_device(self._h, d_patterns, d_offsets, nq, int(total_bytes), d_ms, d_ranges, d_fallbacks, d_prof, stream))

    def count_kmers(self, k, include_Ns=False, force=False):
        """`countKMers` (reference src/algorithms.cpp:387-421)."""
        res = C.c_uint64()
        _check(self._L.gcsa2_count_kmers(self._h, k, int(include_Ns), int(force), C.byref(res)))
        return res.value

    # ---- samples (gcsa.h:191-210) ---------------------------------------------------------
    def sample_range_batch(self, nodes):
        nodes = np.ascontiguousarray(nodes, dtype=np.uint64)
        out = np.zeros((nodes.shape[0], 3), dtype=np.uint64)
        _check(self._L.gcsa2_sample_range_batch(self._h, _p64(nodes), nodes.shape[0], _p64(out)))
        return out

    def sampled(self, node):
        return bool(self.sample_range_batch([node])[0, 0])

    def sampleRange(self, node):
        r = self.sample_range_batch([node])[0]
        return (int(r[1]), int(r[2]))

    def firstSample(self, node):
        return int(self.sample_range_batch([node])[0, 1])

    def sample_batch(self, idx):
        idx = np.ascontiguousarray(idx, dtype=np.uint64)
        values = np.zeros(idx.shape[0], dtype=np.uint64)
        last = np.zeros(idx.shape[0], dtype=np.uint8)
        _check(self._L.gcsa2_sample_batch(self._h, _p64(idx), idx.shape[0], _p64(values), _p8(last)))
        return values, last.astype(bool)

    def sample(self, i):
        return int(self.sample_batch([i])[0][0])

    def lastSample(self, i):
        return bool(self.sample_batch([i])[1][0])

    def sampledPositions(self):
        return int(self._L.gcsa2_sampled_positions(self._h))

    def locate_device(self, d_ranges, nq, stream=0, sort=True):
        """Returns (job, d_offsets, d_values, total); free with locate_discard(job)."""
        job, d_off, d_val = C.c_void_p(), C.c_void_p(), C.c_void_p()
        total = C.c_uint64()
        _check(self._L.gcsa2_locate_device(self._h, d_ranges, nq, int(sort), C.byref(job), C.byref(d_off),
                                           C.byref(d_val), C.byref(total), stream))
        return job, d_off.value, d_val.value, total.value

    def locate_discard(self, job):
        self._L.gcsa2_locate_discard(job)

    def locate_into(self, d_ranges, nq, d_offsets, d_values, capacity, stream=0, sort=True):
        """locate() into caller-owned device buffers; returns the number of values.  Raises
        Gcsa2Error (BUFFER_TOO_SMALL, `.needed` = values required) when capacity is insufficient."""
        total = C.c_uint64()
        rc = self._L.gcsa2_locate_into(self._h, d_ranges, nq, int(sort), d_offsets, d_values, capacity, C.byref(total), stream)
        if rc != 0:
            err = Gcsa2Error(rc, self._L.gcsa2_last_error().decode(errors="replace"))
            err.needed = total.value
            raise err
        return total.value

    def locate_max_into(self, d_ranges, nq, max_positions, d_offsets, d_values, capacity, stream=0):
        """locate(range, max_positions) of nq device ranges into caller-owned device buffers; returns the number of values.
        Raises Gcsa2Error (BUFFER_TOO_SMALL, `.needed` = values required) when capacity is insufficient."""
        total = C.c_uint64()
        rc = self._L.gcsa2_locate_max_into(self._h, d_ranges, nq, int(max_positions), d_offsets, d_values, capacity,
                                           C.byref(total), stream)
        if rc != 0:
            err = Gcsa2Error(rc, self._L.gcsa2_last_error().decode(errors="replace"))
            err.needed = total.value
            raise err
        return total.value

    def count_device(self, d_ranges, nq, d_counts, stream=0):
        _check(self._L.gcsa2_count_device(self._h, d_ranges, nq, d_counts, stream))

    def lf_device(self, d_in, d_comps, nq, d_out, stream=0):
        _check(self._L.gcsa2_lf_device(self._h, d_in, d_comps, nq, d_out, stream))

    def parent_device(self, d_ranges, nq, d_nodes, stream=0):
        _check(self._L.gcsa2_parent_device(self._h, d_ranges, nq, d_nodes, stream))


class LCPArray:
    """`gcsa::LCPArray` queries (reference include/gcsa/lcp.h:137-178) over the LCP part of the
    same device image as a `GCSA`."""

    def __init__(self, gcsa: GCSA, lcp_values: int, lcp_size: int):
        self._g = gcsa
        self._L = gcsa._L
        self._values = int(lcp_values)
        self._size = int(lcp_size)

    def size(self):
        return self._size

    def values(self):
        return self._values

    def notFound(self):
        return (self._values, self._values)

    def root(self):
        return (0, self._size - 1, 0, 0, 0)

    def parent_batch(self, ranges):
        ranges = _ranges(ranges)
        out = np.zeros(ranges.shape[0], dtype=STNODE_DTYPE)
        _check(self._L.gcsa2_parent_batch(self._g.handle, _p64(ranges), ranges.shape[0], out.ctypes.data))
        return out

    def parent(self, rng):
        return tuple(int(x) for x in self.parent_batch(np.array([rng], dtype=np.uint64))[0])

    def depth_batch(self, ranges):
        ranges = _ranges(ranges)
        out = np.zeros(ranges.shape[0], dtype=np.uint64)
        _check(self._L.gcsa2_depth_batch(self._g.handle, _p64(ranges), ranges.shape[0], _p64(out)))
        return out

    def depth(self, rng):
        return int(self.depth_batch(np.array([rng], dtype=np.uint64))[0])

    def _sv_batch(self, op, positions):
        positions = np.ascontiguousarray(positions, dtype=np.uint64)
        out = np.zeros((positions.shape[0], 2), dtype=np.uint64)
        _check(self._L.gcsa2_sv_batch(self._g.handle, op, _p64(positions), positions.shape[0], _p64(out)))
        return out

    def psv_batch(self, positions):
        return self._sv_batch(0, positions)

    def psev_batch(self, positions):
        return self._sv_batch(1, positions)

    def nsv_batch(self, positions):
        return self._sv_batch(2, positions)

    def nsev_batch(self, positions):
        return self._sv_batch(3, positions)

    def psv(self, pos):
        return tuple(int(x) for x in self._sv_batch(0, [pos])[0])

    def psev(self, pos):
        return tuple(int(x) for x in self._sv_batch(1, [pos])[0])

    def nsv(self, pos):
        return tuple(int(x) for x in self._sv_batch(2, [pos])[0])

    def nsev(self, pos):
        return tuple(int(x) for x in self._sv_batch(3, [pos])[0])

    def rmq_batch(self, ranges):
        ranges = _ranges(ranges)
        out = np.zeros((ranges.shape[0], 2), dtype=np.uint64)
        _check(self._L.gcsa2_rmq_batch(self._g.handle, _p64(ranges), ranges.shape[0], _p64(out)))
        return out

    def rmq(self, sp, ep):
        return tuple(int(x) for x in self.rmq_batch(np.array([[sp, ep]], dtype=np.uint64))[0])

    def levels(self):
        return int(self._L.gcsa2_lcp_levels(self._g.handle))

    def branching(self):
        return int(self._L.gcsa2_lcp_branching(self._g.handle))

    def access_batch(self, positions):
        positions = np.ascontiguousarray(positions, dtype=np.uint64)
        out = np.zeros(positions.shape[0], dtype=np.uint64)
        _check(self._L.gcsa2_lcp_access_batch(self._g.handle, _p64(positions), positions.shape[0], _p64(out)))
        return out

    def __getitem__(self, i):
        return int(self.access_batch([i])[0])

    def nodeFor(self, rng):
        """LCPArray::nodeFor (lcp.h:163-175)."""
        sp, ep = int(rng[0]), int(rng[1])
        right = self[ep + 1] if ep + 1 < self._size else 0
        return (sp, ep, self[sp], right, UNKNOWN)


class Comm:
    """RCCL communicator of the library (`gcsa2_comm_*`): one rank per GPU, one gather of hit ranges on the root.
    The 128-byte id is made on one rank (`Comm.unique_id()`) and handed to the others by the launcher."""

    ID_BYTES = 128

    @staticmethod
    def unique_id() -> bytes:
        buf = np.zeros(Comm.ID_BYTES, dtype=np.uint8)
        _check(load_library().gcsa2_comm_unique_id(_p8(buf)))
        return buf.tobytes()

    def __init__(self, unique_id: bytes, rank: int, world: int, device: int):
        self._L = load_library()
        buf = np.frombuffer(unique_id, dtype=np.uint8).copy()
        assert buf.shape[0] == Comm.ID_BYTES
        h = C.c_void_p()
        _check(self._L.gcsa2_comm_create(_p8(buf), rank, world, device, C.byref(h)))
        self._h = h
        self.rank, self.world = rank, world

    GATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p, C.c_int, C.c_void_p)

    @classmethod
    def custom(cls, rank: int, world: int, device: int, gather):
        """A communicator over the application's own transport (gcsa2_comm_create_custom): `gather(d_send, sizes, d_recv, root,
        stream) -> int` with device pointers as integers and `sizes` the list of bytes per rank; 0 = success.  Everything above
        the transport -- sharded matching statistics, sharded locate() with its CSR rebasing -- is the library's C++ as with
        RCCL (gcsa2_amd/host_transport.py holds a gather through host memory over torch.distributed)."""
        self = cls.__new__(cls)
        self._L = load_library()
        self.rank, self.world = rank, world

        def trampoline(user, d_send, sizes, d_recv, root, stream):
            try:
                return int(gather(d_send or 0, [int(sizes[r]) for r in range(world)], d_recv or 0, int(root), stream or 0))
            except Exception as e:                   # an exception must not cross the C frames
                print(f"gcsa2 custom gather failed on rank {rank}: {e!r}", file=sys.stderr, flush=True)
                return 1
        self._callback = Comm.GATHER_FN(trampoline)             # kept alive with the communicator
        h = C.c_void_p()
        _check(self._L.gcsa2_comm_create_custom(rank, world, device, C.cast(self._callback, C.c_void_p), None, C.byref(h)))
        self._h = h
        return self

    def rccl_ranks(self) -> int:
        """The number of ranks RCCL itself reports for this communicator (ncclCommCount)."""
        n = C.c_int(0)
        _check(self._L.gcsa2_comm_rccl_ranks(self._h, C.byref(n)))
        return n.value

    def gather(self, d_send, bytes_per_rank, d_recv, root=0, stream=0):
        """Enqueue the gather: rank r sends bytes_per_rank[r] bytes from device pointer d_send; the root receives
        all parts back to back at device pointer d_recv."""
        sizes = np.asarray(bytes_per_rank, dtype=np.uint64)
        assert sizes.shape[0] == self.world
        _check(self._L.gcsa2_comm_gather(self._h, d_send, _p64(sizes), d_recv, root, stream))

    def match_stats(self, gcsa, d_patterns, d_offsets, counts, pattern_bytes, d_ms_root, d_ranges_root, d_fallbacks_root, root=0, stream=0):
        """Matching statistics of this rank's shard, gathered on the root in query order (enqueue-only).  counts[r] /
        pattern_bytes[r] = patterns / pattern bytes of rank r's shard; the *_root pointers are read on the root only."""
        cnt, pb = np.asarray(counts, dtype=np.uint64), np.asarray(pattern_bytes, dtype=np.uint64)
        assert cnt.shape[0] == self.world and pb.shape[0] == self.world
        _check(self._L.gcsa2_comm_match_stats(self._h, gcsa.handle, d_patterns, d_offsets, _p64(cnt), _p64(pb), root, d_ms_root, d_ranges_root,
                                              d_fallbacks_root, stream))

    def locate(self, gcsa, d_ranges, counts, d_offsets_root, root=0, stream=0, sort=True):
        """locate() of this rank's shard; on the root returns (job, d_values, total) for the whole batch in query order
        (offsets written to d_offsets_root: sum(counts) + 1 entries; free the job with gcsa.locate_discard), None elsewhere."""
        cnt = np.asarray(counts, dtype=np.uint64)
        assert cnt.shape[0] == self.world
        job, d_val, total = C.c_void_p(), C.c_void_p(), C.c_uint64()
        _check(self._L.gcsa2_comm_locate(self._h, gcsa.handle, d_ranges, _p64(cnt), int(sort), root, d_offsets_root, C.byref(job), C.byref(d_val),
                                         C.byref(total), stream))
        return (job, d_val.value, total.value) if self.rank == root else None

    def close(self):
        if getattr(self, "_h", None):
            self._L.gcsa2_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


def fetch_job(job, total: int) -> np.ndarray:
    """The values of a locate job (gcsa2_locate_device / group / comm locate) on the host; frees the job (gcsa2_locate_fetch)."""
    values = np.zeros(max(int(total), 1), dtype=np.uint64)
    _check(load_library().gcsa2_locate_fetch(job, _p64(values), values.shape[0]))
    return values[: int(total)]


def pack_ranges32_device(d_ranges, nq, d_packed, stream=0):
    _check(load_library().gcsa2_pack_ranges32_device(d_ranges, nq, d_packed, stream))


def unpack_ranges32_device(d_packed, nq, d_ranges, stream=0):
    _check(load_library().gcsa2_unpack_ranges32_device(d_packed, nq, d_ranges, stream))


def pack_ranges40_device(d_ranges, nq, d_packed, stream=0):
    _check(load_library().gcsa2_pack_ranges40_device(d_ranges, nq, d_packed, stream))


def unpack_ranges40_device(d_packed, nq, d_ranges, stream=0):
    _check(load_library().gcsa2_unpack_ranges40_device(d_packed, nq, d_ranges, stream))


def wire48_bytes(nq, capacity):
    """Size of a shard's block in the six-byte wire format: nq ranges and an overflow list of `capacity` entries."""
    return int(load_library().gcsa2_wire48_bytes(nq, capacity))


def pack_ranges48_device(d_ranges, nq, d_packed, capacity, stream=0):
    _check(load_library().gcsa2_pack_ranges48_device(d_ranges, nq, d_packed, capacity, stream))


def unpack_ranges48_device(d_packed, nq, capacity, d_ranges, d_overflow_count=0, stream=0):
    _check(load_library().gcsa2_unpack_ranges48_device(d_packed, nq, capacity, d_ranges, d_overflow_count, stream))


class GCSAGroup:
    """One replica per device; `find_batch` shards the batch contiguously over the replicas
    (single-process multi-GPU, `gcsa2_group_*`)."""

    def __init__(self, index_arrays, devices):
        L = load_library()
        holder = make_host_view(index_arrays)
        devs = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        _check(L.gcsa2_group_create(holder.ref(), devs, len(devices), C.byref(h)))
        self._h, self._L = h, L

    def size(self):
        return int(self._L.gcsa2_group_size(self._h))

    def find_batch(self, patterns, offsets, out=None):
        """`out`: an (nq, 2) uint64 array to receive the ranges (a caller that reuses its result buffer avoids the page
        faults of a fresh one, which cost as much as the batch itself at 10 M queries)."""
        patterns = np.ascontiguousarray(patterns, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        nq = offsets.shape[0] - 1
        if out is None:
            out = np.zeros((nq, 2), dtype=np.uint64)
        assert out.dtype == np.uint64 and out.shape == (nq, 2) and out.flags["C_CONTIGUOUS"]
        _check(self._L.gcsa2_group_find_batch(self._h, _p8(patterns), _p64(offsets), nq, _p64(out)))
        return out

    def uses_rccl(self):
        return bool(self._L.gcsa2_group_uses_rccl(self._h))

    def find_device(self, d_patterns, d_offsets, counts, d_ranges_root):
        """Shards already in HBM: d_patterns[r] / d_offsets[r] are device pointers on the device of replica r,
        d_ranges_root a device pointer on the device of replica 0 (2 x sum(counts) words); complete on return."""
        G = self.size()
        assert len(d_patterns) == G and len(d_offsets) == G and len(counts) == G
        pats = (C.c_void_p * G)(*[C.c_void_p(int(p)) for p in d_patterns])
        offs = (C.c_void_p * G)(*[C.c_void_p(int(p)) for p in d_offsets])
        cnt = np.asarray(counts, dtype=np.uint64)
        _check(self._L.gcsa2_group_find_device(self._h, pats, offs, _p64(cnt), d_ranges_root))

    def match_stats_device(self, d_patterns, d_offsets, counts, pattern_bytes, d_ms_root, d_ranges_root, d_fallbacks_root=0):
        """Matching statistics of a batch sharded over the replicas (shards in HBM as for find_device; pattern_bytes[r] =
        pattern bytes of shard r); statistics, ranges and parent() counts gathered on replica 0's device.  Complete on return."""
        G = self.size()
        pats = (C.c_void_p * G)(*[C.c_void_p(int(p)) for p in d_patterns])
        offs = (C.c_void_p * G)(*[C.c_void_p(int(p)) for p in d_offsets])
        cnt, pb = np.asarray(counts, dtype=np.uint64), np.asarray(pattern_bytes, dtype=np.uint64)
        _check(self._L.gcsa2_group_match_stats_device(self._h, pats, offs, _p64(cnt), _p64(pb), d_ms_root, d_ranges_root, d_fallbacks_root))

    def locate_device(self, d_ranges, counts, d_offsets_root, sort=True):
        """locate() of a batch of ranges sharded over the replicas; returns (job, d_values, total) on replica 0's device,
        offsets of the whole batch in d_offsets_root (sum(counts) + 1 entries).  Free with locate_discard(job)."""
        G = self.size()
        rng = (C.c_void_p * G)(*[C.c_void_p(int(p)) for p in d_ranges])
        cnt = np.asarray(counts, dtype=np.uint64)
        job, d_val, total = C.c_void_p(), C.c_void_p(), C.c_uint64()
        _check(self._L.gcsa2_group_locate_device(self._h, rng, _p64(cnt), int(sort), d_offsets_root, C.byref(job), C.byref(d_val), C.byref(total)))
        return job, d_val.value, total.value

    def locate_discard(self, job):
        self._L.gcsa2_locate_discard(job)

    def close(self):
        if getattr(self, "_h", None):
            self._L.gcsa2_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def serialize_view(view_ref, what="gcsa") -> bytes:
    """GCSA::serialize / LCPArray::serialize of a host view (`gcsa2_host_view_serialize_*`) as bytes."""
    L = load_library()
    chunks = []
    sink = SINK(lambda ctx, data, n: chunks.append(C.string_at(data, n)))
    fn = L.gcsa2_host_view_serialize_gcsa if what == "gcsa" else L.gcsa2_host_view_serialize_lcp
    written = C.c_uint64()
    _check(fn(view_ref, sink, None, C.byref(written)))
    out = b"".join(chunks)
    assert len(out) == written.value
    return out


def parse_view(data: bytes, what="gcsa", exact=True):
    """`gcsa2_host_view_parse_*`: (storage handle, HostView pointer, bytes consumed); free with free_view()."""
    L = load_library()
    buf = C.create_string_buffer(data, len(data))
    h = C.c_void_p()
    consumed = C.c_uint64()
    fn = L.gcsa2_host_view_parse_gcsa if what == "gcsa" else L.gcsa2_host_view_parse_lcp
    _check(fn(buf, len(data), None if exact else C.byref(consumed), C.byref(h)))
    return h, L.gcsa2_host_view_get(h), (len(data) if exact else consumed.value)


def free_view(h):
    load_library().gcsa2_host_view_free(h)


def open_index(index_arrays, device=0):
    """(GCSA, LCPArray) over one device image; `index_arrays` may be an IndexArrays, a G2HV file or a
    `.gcsa` file with its `.lcp` beside it."""
    g = GCSA(index_arrays, device=device)
    lcp = LCPArray(g, int(g._L.gcsa2_lcp_values(g.handle)), int(g._L.gcsa2_lcp_size(g.handle)))
    return g, lcp
