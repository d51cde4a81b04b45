"""supersampler_amd -- Python host mirror of libspsp (include/spsp.h).

A thin ctypes layer over the C-ABI: every GPU entry point goes straight to the
HIP kernels in libspsp.so; there is no Python or CPU fallback.  Loading fails
loudly if the shared library has not been built
(`python -c "import __graft_entry__ as g; g.build()"` or `make -C supersampler_amd/csrc`).

If the process also uses PyTorch, import torch BEFORE this package: torch
ships its own libamdhip64.so.7 and the first HIP runtime loaded is the one both
share.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SPSP_LIB: A/B experiments with another build (tools/ab_small.sh).  Whatever is loaded is reported: library_info() goes
# into bench.py's JSON line and the pytest header, and an override is announced on stderr when it is loaded.
LIB_OVERRIDDEN = bool(os.environ.get("SPSP_LIB"))
LIB_PATH = os.environ.get("SPSP_LIB") or os.path.join(_HERE, "libspsp.so")

SPSP_SCAN_DEFAULT = 0
SPSP_SCAN_DIRECT_HASH = 1
SPSP_SCAN_LDS_FILTER = 2
SPSP_SCAN_PAIR_FILTER = 4
SPSP_SCAN_STATS = 8
SPSP_SCAN_BLOOM_FILTER = 16
SPSP_SCAN_PACKED_INPUT = 32


class SpspError(RuntimeError):
    code = 0


ERR_OVERFLOW = -7
KEYS_UNORDERED = 1
ERR_ARG, ERR_FORMAT = -1, -6
RATE_AS_IS, RATE_COARSEST = 0.0, -1.0      # compare_files(rate=...): the headers' rates ignored / the coarsest of the files' ("auto")
TIME_DENSE, TIME_SCAN, TIME_ACCUMULATE, TIME_COMPARE, TIME_PARTS, TIME_ALL = 1, 2, 4, 8, 16, 31


class Params(C.Structure):
    _fields_ = [("k", C.c_uint32), ("m", C.c_uint32), ("threshold", C.c_uint64),
                ("abundance", C.c_uint32), ("flags", C.c_uint32)]


class SketchView(C.Structure):
    _fields_ = [("minimizer", C.c_void_p), ("kmer_lo", C.c_void_p), ("kmer_hi", C.c_void_p), ("n", C.c_uint64)]


class SketchStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in
                ("read_kmer", "selected_kmer_number", "selected_superkmer_number", "count_maximal_skmer",
                 "seen_kmers_at_reconstruction", "seen_superkmers_at_reconstruction",
                 "seen_max_superkmers_at_reconstruction", "actual_minimizer_number", "nb_mmer_selected",
                 "total_kmer_number", "total_superkmer_number")]


class Timing(C.Structure):
    _fields_ = [("dense_ms", C.c_double), ("dense_launches", C.c_uint64), ("scan_ms", C.c_double),
                ("scan_calls", C.c_uint64), ("accumulate_ms", C.c_double), ("accumulate_launches", C.c_uint64),
                ("compare_ms", C.c_double), ("compare_calls", C.c_uint64),
                ("scatter_ms", C.c_double), ("scatter_launches", C.c_uint64),
                ("group_ms", C.c_double), ("group_launches", C.c_uint64)]


class StageTimes(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("read_s", "ingest_s", "scan_s", "gather_s", "build_s", "gzip_s", "load_s",
                                          "compare_s", "csv_s", "csv_gzip_s")] + [("sketch_files", C.c_uint64), ("compare_calls", C.c_uint64)]


class HbmRates(C.Structure):
    _fields_ = [("copy_GBps", C.c_double), ("copy_ms", C.c_double), ("read_GBps", C.c_double), ("read_ms", C.c_double),
                ("bytes", C.c_uint64), ("reps", C.c_uint32), ("n_cu", C.c_uint32)]


class GatherRow(C.Structure):
    """spsp_gather_row: one named reference of one query (include/spsp.h)"""
    _fields_ = [("query", C.c_uint32), ("rank", C.c_uint32), ("match", C.c_uint32), ("reserved", C.c_uint32),
                ("intersect", C.c_uint64), ("unique", C.c_uint64), ("remaining", C.c_uint64)]


GATHER_ROW_DTYPE = np.dtype([("query", "<u4"), ("rank", "<u4"), ("match", "<u4"), ("reserved", "<u4"), ("intersect", "<u8"), ("unique", "<u8"),
                             ("remaining", "<u8")])

class ClusterRow(C.Structure):
    """spsp_cluster_row: one sketch's place in the clustering of its collection (include/spsp.h)"""
    _fields_ = [("cluster", C.c_uint32), ("representative", C.c_uint32), ("size", C.c_uint32), ("reserved", C.c_uint32), ("shared", C.c_uint64)]


CLUSTER_ROW_DTYPE = np.dtype([("cluster", "<u4"), ("representative", "<u4"), ("size", "<u4"), ("reserved", "<u4"), ("shared", "<u8")])
CLUSTER_JACCARD, CLUSTER_CONTAINMENT = 0, 1


class NeighbourRow(C.Structure):
    """spsp_neighbour_row: one partner in one sketch's list of best matches (include/spsp.h)"""
    _fields_ = [("sketch", C.c_uint32), ("rank", C.c_uint32), ("neighbour", C.c_uint32), ("reserved", C.c_uint32), ("shared", C.c_uint64)]


NEIGHBOUR_ROW_DTYPE = np.dtype([("sketch", "<u4"), ("rank", "<u4"), ("neighbour", "<u4"), ("reserved", "<u4"), ("shared", "<u8")])
NEIGHBOUR_JACCARD, NEIGHBOUR_CONTAINMENT, NEIGHBOUR_CONTAINED = 0, 1, 2

class BatchFile(C.Structure):
    """spsp_batch_file: one file's place in the slab of spsp_ingest_batch (include/spsp.h)"""
    _fields_ = [("off", C.c_uint64), ("text_len", C.c_uint64), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


BATCH_FASTQ, BATCH_FAILED = 1, 2


class TreeRow(C.Structure):
    """spsp_tree_row: one merge of a collection's single-linkage tree (include/spsp.h)"""
    _fields_ = [("a", C.c_uint32), ("b", C.c_uint32), ("size", C.c_uint32), ("reserved", C.c_uint32), ("shared", C.c_uint64)]


TREE_ROW_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("size", "<u4"), ("reserved", "<u4"), ("shared", "<u8")])

# spsp_prevalence_row: a row sketch's keys by class of holder count, and the sum of the holder counts (include/spsp.h)
PREVALENCE_ROW_DTYPE = np.dtype([("core", "<u8"), ("shell", "<u8"), ("unique", "<u8"), ("absent", "<u8"), ("holders", "<u8")])

# spsp_accumulation_row: pan and core at one step of the curves -- minimum, maximum and sum over the orders, and order 0's (include/spsp.h)
ACCUMULATION_ROW_DTYPE = np.dtype([("pan_min", "<u8"), ("pan_max", "<u8"), ("pan_sum", "<u8"), ("core_min", "<u8"), ("core_max", "<u8"),
                                   ("core_sum", "<u8"), ("pan_first", "<u8"), ("core_first", "<u8")])

# spsp_group_row / spsp_group_member_row: a group's distinct keys by kind, and a member's own keys by kind (include/spsp.h)
GROUP_ROW_DTYPE = np.dtype([("members", "<u8"), ("entries", "<u8"), ("present", "<u8"), ("core", "<u8"), ("exclusive", "<u8"), ("marker", "<u8")])
GROUP_MEMBER_ROW_DTYPE = np.dtype([("core", "<u8"), ("exclusive", "<u8"), ("marker", "<u8")])

# spsp_classify_record / spsp_classify_hit: a record's counts, and one of its listed matches (include/spsp.h)
CLASSIFY_RECORD_DTYPE = np.dtype([("length", "<u8"), ("keys", "<u4"), ("hit_keys", "<u4"), ("passing", "<u4"), ("listed", "<u4")])
CLASSIFY_HIT_DTYPE = np.dtype([("reference", "<u4"), ("shared", "<u4")])

# spsp_depth_row / spsp_depth_totals: a reference's depth statistics, and the read set's totals (include/spsp.h)
DEPTH_ROW_DTYPE = np.dtype([("sum", "<u8"), ("unique_sum", "<u8"), ("keys", "<u4"), ("found", "<u4"), ("median", "<u4"), ("max", "<u4"),
                            ("unique_keys", "<u4"), ("unique_found", "<u4"), ("unique_median", "<u4"), ("unique_max", "<u4")])
DEPTH_TOTALS_DTYPE = np.dtype([("record_keys", "<u8"), ("hit_keys", "<u8"), ("index_keys", "<u4"), ("index_found", "<u4")])

# spsp_profile_row / spsp_profile_totals: one round of the profile (rank = its place + 1), and the call's totals (include/spsp.h)
PROFILE_ROW_DTYPE = np.dtype([("sum", "<u8"), ("reference", "<u4"), ("keys", "<u4"), ("found", "<u4"), ("assigned", "<u4"), ("median", "<u4"), ("max", "<u4"),
                              ("remaining", "<u4"), ("reserved", "<u4")])
PROFILE_TOTALS_DTYPE = np.dtype([("found_sum", "<u8"), ("assigned_sum", "<u8"), ("found_keys", "<u4"), ("assigned_keys", "<u4")])

# spsp_taxonomy_record: a record's call in the tree of the index's taxonomy (include/spsp.h)
TAXONOMY_RECORD_DTYPE = np.dtype([("length", "<u8"), ("keys", "<u4"), ("hit_keys", "<u4"), ("node", "<u4"), ("start", "<u4"), ("score", "<u4"),
                                  ("clade", "<u4"), ("direct", "<u4"), ("winners", "<u4")])
TAXONOMY_NONE = 0xffffffff

# spsp_segment_row / spsp_mosaic_row: a stretch of a record with one call, and a record's line of a windowed run (include/spsp.h)
SEGMENT_ROW_DTYPE = np.dtype([("begin", "<u8"), ("end", "<u8"), ("keys", "<u8"), ("hit_keys", "<u8"), ("support", "<u8"), ("record", "<u4"), ("segment", "<u4"),
                              ("windows", "<u4"), ("call", "<u4")])
MOSAIC_ROW_DTYPE = np.dtype([("length", "<u8"), ("major_bases", "<u8"), ("second_bases", "<u8"), ("keys", "<u8"), ("hit_keys", "<u8"), ("windows", "<u4"),
                             ("segments", "<u4"), ("called_windows", "<u4"), ("calls", "<u4"), ("major", "<u4"), ("major_windows", "<u4"), ("second", "<u4"),
                             ("second_windows", "<u4")])
WINDOWS_ABSENT = 0xffffffff

FILE_CALLBACK = C.CFUNCTYPE(None, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.POINTER(SketchStats), C.c_char_p)

SUPERKMER_DTYPE = np.dtype([("rec", "<u4"), ("minimizer", "<u4"), ("start", "<u8"), ("len", "<u4"), ("rev", "<u4")])

# every symbol include/spsp.h declares (tests check the .so exports them all)
ABI_SYMBOLS = [
    "spsp_device_count", "spsp_create", "spsp_destroy", "spsp_last_error", "spsp_version", "spsp_free", "spsp_copy_to_host",
    "spsp_stream_create_cus", "spsp_stream_destroy", "spsp_set_cu_count", "spsp_pack_bases_device",
    "spsp_timing_enable", "spsp_timing_sample", "spsp_timing_read", "spsp_threshold_host", "spsp_scan", "spsp_scan_device", "spsp_scan_device_begin", "spsp_scan_device_end", "spsp_scan_tail_stream", "spsp_wait_dense", "spsp_wait_stream", "spsp_scan_hits_device", "spsp_count_superkmers_device", "spsp_stats_counts", "spsp_compare",
    "spsp_compare_device", "spsp_slot_bytes", "spsp_partition_keys_device", "spsp_compare_slots_device", "spsp_compare_device_begin", "spsp_compare_slots_device_begin", "spsp_compare_end", "spsp_fasta_clean_host", "spsp_fasta_clean_device", "spsp_fasta_clean_packed_device", "spsp_fastq_clean_device", "spsp_fastq_clean_packed_device", "spsp_ingest_batch", "spsp_sketch_text", "spsp_sketch_build_host", "spsp_sketch_build_device", "spsp_sketch_parse_host", "spsp_sketch_decode_device", "spsp_sketch_keys_device", "spsp_sketch_keys_device_begin", "spsp_sketch_keys_device_end", "spsp_sketch_keys_big_genomes", "spsp_scan_output_wait", "spsp_compare_keys_unordered", "spsp_compare_forget", "spsp_sketch_chain_host",
    "spsp_csv_host", "spsp_csv_cells_host", "spsp_csv_cells_gz_host", "spsp_sort_csv_host", "spsp_read_file_host", "spsp_write_gz_host", "spsp_sketch_file", "spsp_compare_files", "spsp_compare_files_chatty", "spsp_stage_times_read", "spsp_measure_hbm_device", "spsp_sketch_files", "spsp_sketch_files_multi", "spsp_sketch_files_release", "spsp_compare_files_multi", "spsp_matrix_cells_device", "spsp_matrix_add_cells_device", "spsp_compare_cells_device", "spsp_compare_slots_cells_device",
    "spsp_keys_downsample_device", "spsp_sketch_header_host", "spsp_sketch_downsample_host", "spsp_compare_files_rate", "spsp_compare_files_multi_rate",
    "spsp_gather_device", "spsp_gather_csv_host", "spsp_gather_files",
    "spsp_cluster_cells_device", "spsp_cluster_csv_host", "spsp_cluster_files",
    "spsp_representatives_cells_device", "spsp_representatives_files",
    "spsp_neighbours_cells_device", "spsp_neighbours_csv_host", "spsp_neighbours_files",
    "spsp_prevalence_device", "spsp_prevalence_csv_host", "spsp_spectrum_csv_host", "spsp_prevalence_files",
    "spsp_tree_cells_device", "spsp_tree_cut_host", "spsp_tree_csv_host", "spsp_tree_newick_host", "spsp_tree_files",
    "spsp_keys_select_device", "spsp_select_band_host", "spsp_sketch_from_keys_host", "spsp_select_files",
    "spsp_accumulation_orders_host", "spsp_accumulation_plan_host", "spsp_accumulation_device", "spsp_accumulation_csv_host", "spsp_accumulation_files",
    "spsp_groups_labels_host", "spsp_groups_bounds_host", "spsp_groups_device", "spsp_groups_csv_host", "spsp_groups_members_csv_host", "spsp_groups_files",
    "spsp_classify_index_device", "spsp_classify_device", "spsp_classify_plan_host", "spsp_classify_csv_host", "spsp_classify_summary_csv_host", "spsp_classify_files", "spsp_classify_stage_ms",
    "spsp_depth_begin_device", "spsp_depth_add_device", "spsp_depth_read_device", "spsp_depth_plan_host", "spsp_depth_stage_ms", "spsp_depth_csv_host", "spsp_depth_files",
    "spsp_profile_device", "spsp_profile_stage_ms", "spsp_profile_counts", "spsp_profile_csv_host", "spsp_profile_files",
    "spsp_taxonomy_lineages_host", "spsp_taxonomy_check_host", "spsp_taxonomy_plan_host", "spsp_taxonomy_index_device", "spsp_taxonomy_device", "spsp_taxonomy_stage_ms", "spsp_taxonomy_csv_host", "spsp_taxonomy_report_csv_host", "spsp_taxonomy_files",
    "spsp_extract_plan_host", "spsp_records_extents_host", "spsp_records_extract_host", "spsp_extract_flags_classify_host", "spsp_extract_flags_taxonomy_host",
    "spsp_extract_word_check_host", "spsp_records_extents_device", "spsp_records_extract_device", "spsp_extract_stage_ms", "spsp_classify_files_extract",
    "spsp_taxonomy_files_extract",
    "spsp_split_plan_host", "spsp_records_split_host", "spsp_split_bins_classify_host", "spsp_split_bins_taxonomy_host", "spsp_split_word_check_host",
    "spsp_split_csv_host", "spsp_records_split_device", "spsp_split_stage_ms", "spsp_classify_files_split", "spsp_taxonomy_files_split",
    "spsp_pairs_names_host", "spsp_union_plan_host", "spsp_records_union_device", "spsp_union_stage_ms", "spsp_classify_files_paired", "spsp_taxonomy_files_paired",
    "spsp_windows_plan_host", "spsp_records_windows_host", "spsp_windows_expand_host", "spsp_windows_segments_host", "spsp_segments_csv_host", "spsp_mosaic_csv_host",
    "spsp_windows_word_check_host", "spsp_records_windows_device", "spsp_windows_stage_ms", "spsp_classify_files_windows", "spsp_taxonomy_files_windows",
    "spsp_segments_plan_host", "spsp_windows_smooth_host", "spsp_segments_word_check_host", "spsp_segments_select_host", "spsp_segments_fasta_host",
    "spsp_segments_write_device", "spsp_segments_stage_ms", "spsp_classify_files_segments", "spsp_taxonomy_files_segments",
    "spsp_lift_plan_host", "spsp_records_lift_host", "spsp_segments_bed_host", "spsp_records_lift_device", "spsp_lift_stage_ms", "spsp_classify_files_raw",
    "spsp_taxonomy_files_raw",
]

_lib = None


def lib():
    """Load libspsp.so (once).  Raises SpspError if it is missing -- never falls back."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SpspError("%s not found: build the HIP extension first (make -C supersampler_amd/csrc)" % LIB_PATH)
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    if LIB_OVERRIDDEN:
        import sys
        print("[supersampler_amd] SPSP_LIB is set: loaded %s instead of the in-tree libspsp.so" % LIB_PATH, file=sys.stderr, flush=True)
    u64, u32, vp, cp, dbl, i32 = C.c_uint64, C.c_uint32, C.c_void_p, C.c_char_p, C.c_double, C.c_int
    P = C.POINTER
    L.spsp_device_count.restype = i32; L.spsp_device_count.argtypes = []
    L.spsp_create.restype = i32; L.spsp_create.argtypes = [i32, vp, P(vp)]
    L.spsp_destroy.restype = None; L.spsp_destroy.argtypes = [vp]
    L.spsp_last_error.restype = cp; L.spsp_last_error.argtypes = []
    L.spsp_version.restype = cp; L.spsp_version.argtypes = []
    L.spsp_free.restype = None; L.spsp_free.argtypes = [vp]
    L.spsp_copy_to_host.restype = i32; L.spsp_copy_to_host.argtypes = [vp, vp, vp, u64]
    L.spsp_stream_create_cus.restype = i32; L.spsp_stream_create_cus.argtypes = [i32, u32, u32, P(vp)]
    L.spsp_stream_destroy.restype = i32; L.spsp_stream_destroy.argtypes = [i32, vp]
    L.spsp_set_cu_count.restype = i32; L.spsp_set_cu_count.argtypes = [vp, u32, u32]
    L.spsp_pack_bases_device.restype = i32; L.spsp_pack_bases_device.argtypes = [vp, vp, u64, P(vp)]
    L.spsp_timing_enable.restype = i32; L.spsp_timing_enable.argtypes = [vp, i32]
    L.spsp_timing_read.restype = i32; L.spsp_timing_read.argtypes = [vp, P(Timing)]
    L.spsp_timing_sample.restype = i32; L.spsp_timing_sample.argtypes = [vp, u32]
    L.spsp_threshold_host.restype = u64; L.spsp_threshold_host.argtypes = [u32, u32, dbl]
    L.spsp_scan.restype = i32; L.spsp_scan.argtypes = [vp, P(Params), vp, vp, u32, P(vp), P(u64)]
    L.spsp_scan_device.restype = i32
    L.spsp_scan_device.argtypes = [vp, P(Params), vp, u64, vp, u32, P(vp), P(u64)]
    L.spsp_scan_device_begin.restype = i32
    L.spsp_scan_device_begin.argtypes = [vp, P(Params), vp, u64, vp, u32]
    L.spsp_scan_device_end.restype = i32; L.spsp_scan_device_end.argtypes = [vp, P(vp), P(u64)]
    L.spsp_wait_dense.restype = i32; L.spsp_wait_dense.argtypes = [vp, vp]
    L.spsp_wait_stream.restype = i32; L.spsp_wait_stream.argtypes = [vp, vp]
    L.spsp_compare_device_begin.restype = i32
    L.spsp_compare_device_begin.argtypes = [vp, u32, vp, vp, vp, vp, u32, u32, u32, u32, vp]
    L.spsp_compare_slots_device_begin.restype = i32
    L.spsp_compare_slots_device_begin.argtypes = [vp, u32, vp, u32, u32, u32, vp]
    L.spsp_compare_end.restype = i32; L.spsp_compare_end.argtypes = [vp]
    L.spsp_scan_hits_device.restype = i32
    L.spsp_scan_hits_device.argtypes = [vp, P(Params), vp, u64, P(u64)]
    L.spsp_compare.restype = i32; L.spsp_compare.argtypes = [vp, P(SketchView), u32, u32, vp, vp]
    L.spsp_compare_device.restype = i32
    L.spsp_compare_device.argtypes = [vp, u32, vp, vp, vp, vp, u32, u32, u32, u32, vp]
    L.spsp_slot_bytes.restype = u64; L.spsp_slot_bytes.argtypes = [u32, u32, u32]
    L.spsp_partition_keys_device.restype = i32
    L.spsp_partition_keys_device.argtypes = [vp, u32, vp, vp, vp, vp, u32, u32, u32, vp]
    L.spsp_compare_slots_device.restype = i32
    L.spsp_compare_slots_device.argtypes = [vp, u32, vp, u32, u32, u32, vp]
    L.spsp_fasta_clean_host.restype = i32
    L.spsp_fasta_clean_host.argtypes = [cp, u64, P(vp), P(vp), P(u32)]
    L.spsp_fasta_clean_device.restype = i32
    L.spsp_fasta_clean_device.argtypes = [vp, vp, u64, P(vp), P(u64), P(vp), P(u32)]
    L.spsp_fasta_clean_packed_device.restype = i32
    L.spsp_fasta_clean_packed_device.argtypes = [vp, vp, u64, P(vp), P(u64), P(vp), P(u32)]
    L.spsp_fastq_clean_device.restype = i32
    L.spsp_fastq_clean_device.argtypes = [vp, vp, u64, P(vp), P(u64), P(vp), P(u32)]
    L.spsp_fastq_clean_packed_device.restype = i32
    L.spsp_fastq_clean_packed_device.argtypes = [vp, vp, u64, P(vp), P(u64), P(vp), P(u32)]
    L.spsp_ingest_batch.restype = i32
    L.spsp_ingest_batch.argtypes = [vp, vp, u64, P(BatchFile), u32, i32, P(vp), P(u64), P(vp), P(u32), vp, vp]
    L.spsp_sketch_text.restype = i32
    L.spsp_sketch_text.argtypes = [vp, P(Params), dbl, cp, u64, P(vp), P(u64), P(SketchStats)]
    L.spsp_sketch_build_host.restype = i32
    L.spsp_sketch_build_host.argtypes = [P(Params), dbl, vp, vp, u32, vp, u64, P(vp), P(u64), P(SketchStats)]
    L.spsp_sketch_build_device.restype = i32
    L.spsp_sketch_build_device.argtypes = [vp, P(Params), dbl, vp, vp, u32, vp, u64, vp, u32, i32, P(vp), vp, vp]
    L.spsp_sketch_parse_host.restype = i32
    L.spsp_sketch_parse_host.argtypes = [cp, u64, P(u32), P(u32), P(vp), P(vp), P(vp), P(u64)]
    L.spsp_sketch_chain_host.restype = i32
    L.spsp_sketch_chain_host.argtypes = [cp, u64, u32, u32, C.c_char_p, P(i32), P(u32), P(u64), P(u64)]
    L.spsp_csv_host.restype = i32
    L.spsp_csv_host.argtypes = [i32, P(cp), u32, u32, vp, vp, i32, dbl, P(vp), P(u64)]
    L.spsp_csv_cells_host.restype = i32
    L.spsp_csv_cells_host.argtypes = [i32, P(cp), u32, u32, vp, u64, vp, i32, dbl, P(vp), P(u64)]
    L.spsp_csv_cells_gz_host.restype = i32
    L.spsp_csv_cells_gz_host.argtypes = [i32, P(cp), u32, u32, vp, u64, vp, i32, dbl, cp]
    L.spsp_sort_csv_host.restype = i32
    L.spsp_sort_csv_host.argtypes = [cp, u64, cp, u64, P(vp), P(u64)]
    L.spsp_read_file_host.restype = i32; L.spsp_read_file_host.argtypes = [cp, P(vp), P(u64)]
    L.spsp_write_gz_host.restype = i32; L.spsp_write_gz_host.argtypes = [cp, cp, u64, i32]
    L.spsp_sketch_file.restype = i32
    L.spsp_sketch_file.argtypes = [vp, P(Params), dbl, cp, cp, P(SketchStats)]
    L.spsp_compare_files.restype = i32
    L.spsp_compare_files.argtypes = [vp, P(cp), u32, u32, i32, dbl, cp]
    L.spsp_sketch_keys_device.restype = i32
    L.spsp_sketch_keys_device.argtypes = [vp, P(Params), vp, u64, vp, vp, u64, vp, u32, u32, P(vp), P(vp), P(vp), vp]
    L.spsp_sketch_keys_device_begin.restype = i32
    L.spsp_sketch_keys_device_begin.argtypes = [vp, P(Params), vp, u64, vp, vp, u64, vp, u32, u32]
    L.spsp_compare_keys_unordered.restype = i32; L.spsp_compare_keys_unordered.argtypes = [vp, i32]
    L.spsp_compare_forget.restype = i32; L.spsp_compare_forget.argtypes = [vp]
    L.spsp_sketch_keys_device_end.restype = i32
    L.spsp_sketch_keys_device_end.argtypes = [vp, P(vp), P(vp), P(vp), vp]
    L.spsp_sketch_keys_big_genomes.restype = u32; L.spsp_sketch_keys_big_genomes.argtypes = [vp]
    L.spsp_scan_output_wait.restype = i32; L.spsp_scan_output_wait.argtypes = [vp, vp]
    L.spsp_sketch_decode_device.restype = i32
    L.spsp_sketch_decode_device.argtypes = [vp, P(cp), P(u64), u32, P(u32), P(u32), P(vp), P(vp), P(vp), P(u64)]
    L.spsp_count_superkmers_device.restype = i32
    L.spsp_count_superkmers_device.argtypes = [vp, P(Params), vp, u64, vp, u32, P(u64)]
    L.spsp_stats_counts.restype = i32
    L.spsp_stats_counts.argtypes = [vp, P(u32)]
    L.spsp_scan_tail_stream.restype = i32; L.spsp_scan_tail_stream.argtypes = [vp, i32, vp]
    L.spsp_stage_times_read.restype = i32; L.spsp_stage_times_read.argtypes = [vp, P(StageTimes), i32]
    L.spsp_sketch_files.restype = i32
    L.spsp_sketch_files.argtypes = [i32, P(Params), dbl, P(cp), P(cp), u32, u32, FILE_CALLBACK, vp, P(StageTimes)]
    L.spsp_sketch_files_multi.restype = i32
    L.spsp_sketch_files_multi.argtypes = [P(i32), u32, P(Params), dbl, P(cp), P(cp), u32, u32, FILE_CALLBACK, vp, P(StageTimes)]
    L.spsp_sketch_files_release.restype = None; L.spsp_sketch_files_release.argtypes = [i32]
    L.spsp_measure_hbm_device.restype = i32; L.spsp_measure_hbm_device.argtypes = [vp, u64, u32, P(HbmRates)]
    L.spsp_compare_files_multi.restype = i32
    L.spsp_compare_files_multi.argtypes = [P(i32), u32, P(cp), u32, u32, i32, dbl, cp, i32, P(StageTimes)]
    L.spsp_matrix_cells_device.restype = i32; L.spsp_matrix_cells_device.argtypes = [vp, vp, u32, u32, u32, vp, u64, P(u64)]
    L.spsp_compare_cells_device.restype = i32; L.spsp_compare_cells_device.argtypes = [vp, u32, vp, vp, vp, vp, u32, u32, vp, vp, u64, P(u64)]
    L.spsp_compare_slots_cells_device.restype = i32; L.spsp_compare_slots_cells_device.argtypes = [vp, u32, vp, u32, u32, u32, vp, vp, u64, P(u64)]
    L.spsp_matrix_add_cells_device.restype = i32; L.spsp_matrix_add_cells_device.argtypes = [vp, vp, u32, vp, u64]
    if not LIB_OVERRIDDEN or hasattr(L, "spsp_keys_downsample_device"):      # (an older build named by SPSP_LIB for an A/B run has none of these)
        L.spsp_keys_downsample_device.restype = i32
        L.spsp_keys_downsample_device.argtypes = [vp, u32, u64, vp, vp, vp, vp, u32, P(vp), P(vp), P(vp), vp]
        L.spsp_sketch_header_host.restype = i32; L.spsp_sketch_header_host.argtypes = [cp, u64, P(u32), P(u32), P(u64), P(dbl)]
        L.spsp_sketch_downsample_host.restype = i32; L.spsp_sketch_downsample_host.argtypes = [cp, u64, dbl, P(vp), P(u64)]
        L.spsp_compare_files_rate.restype = i32
        L.spsp_compare_files_rate.argtypes = [vp, P(cp), u32, u32, i32, dbl, cp, i32, dbl]
        L.spsp_compare_files_multi_rate.restype = i32
        L.spsp_compare_files_multi_rate.argtypes = [P(i32), u32, P(cp), u32, u32, i32, dbl, cp, i32, P(StageTimes), dbl]
    if not LIB_OVERRIDDEN or hasattr(L, "spsp_gather_device"):
        L.spsp_gather_device.restype = i32
        L.spsp_gather_device.argtypes = [vp, u32, vp, vp, vp, vp, u32, u32, u64, u32, vp, u64, P(u64)]
        L.spsp_gather_csv_host.restype = i32
        L.spsp_gather_csv_host.argtypes = [vp, u64, P(cp), u32, u32, vp, i32, P(vp), P(u64)]
        L.spsp_gather_files.restype = i32
        L.spsp_gather_files.argtypes = [vp, P(cp), u32, u32, i32, u64, u32, cp, i32, dbl, P(vp), P(u64)]
    if not LIB_OVERRIDDEN or hasattr(L, "spsp_cluster_cells_device"):
        L.spsp_cluster_cells_device.restype = i32
        L.spsp_cluster_cells_device.argtypes = [vp, vp, u64, vp, u32, i32, u32, u32, vp, P(u64), P(u64)]
        L.spsp_cluster_csv_host.restype = i32
        L.spsp_cluster_csv_host.argtypes = [vp, P(cp), u32, vp, i32, i32, P(vp), P(u64)]
        L.spsp_cluster_files.restype = i32
        L.spsp_cluster_files.argtypes = [vp, P(cp), u32, i32, i32, u32, u32, cp, i32, dbl, P(vp), P(u64)]
    if not LIB_OVERRIDDEN or hasattr(L, "spsp_representatives_cells_device"):
        L.spsp_representatives_cells_device.restype = i32
        L.spsp_representatives_cells_device.argtypes = [vp, vp, u64, vp, vp, u32, i32, u32, u32, vp, P(u64), P(u64), P(u32)]
        L.spsp_representatives_files.restype = i32
        L.spsp_representatives_files.argtypes = [vp, P(cp), u32, i32, i32, u32, u32, vp, cp, i32, dbl, P(vp), P(u64)]
    if not LIB_OVERRIDDEN or hasattr(L, "spsp_neighbours_cells_device"):
        L.spsp_neighbours_cells_device.restype = i32
        L.spsp_neighbours_cells_device.argtypes = [vp, vp, u64, vp, u32, u32, i32, u32, u32, u32, vp, u64, P(u64), vp, P(u64)]
        L.spsp_neighbours_csv_host.restype = i32
        L.spsp_neighbours_csv_host.argtypes = [vp, u64, vp, P(cp), u32, u32, vp, i32, i32, P(vp), P(u64)]
        L.spsp_neighbours_files.restype = i32
        L.spsp_neighbours_files.argtypes = [vp, P(cp), u32, u32, i32, i32, u32, u32, u32, cp, i32, dbl, P(vp), P(u64)]
    if not LIB_OVERRIDDEN or hasattr(L, "spsp_prevalence_device"):
        L.spsp_prevalence_device.restype = i32
        L.spsp_prevalence_device.argtypes = [vp, u32, vp, vp, vp, vp, u32, u32, u32, u32, vp, vp, P(vp)]
        L.spsp_prevalence_csv_host.restype = i32
        L.spsp_prevalence_csv_host.argtypes = [vp, u32, P(cp), vp, i32, P(vp), P(u64)]
        L.spsp_spectrum_csv_host.restype = i32
        L.spsp_spectrum_csv_host.argtypes = [vp, u32, P(vp), P(u64)]
        L.spsp_prevalence_files.restype = i32
        L.spsp_prevalence_files.argtypes = [vp, P(cp), u32, u32, i32, u32, u32, cp, i32, dbl, P(vp), P(vp)]
    if not LIB_OVERRIDDEN or hasattr(L, "spsp_tree_cells_device"):
        L.spsp_tree_cells_device.restype = i32
        L.spsp_tree_cells_device.argtypes = [vp, vp, u64, vp, u32, i32, u32, u32, vp, P(u64), P(u64), P(u32)]
        L.spsp_tree_cut_host.restype = i32
        L.spsp_tree_cut_host.argtypes = [vp, u64, u32, vp, i32, u32, u32, u32, u32, vp, P(u64)]
        L.spsp_tree_csv_host.restype = i32
        L.spsp_tree_csv_host.argtypes = [vp, u64, P(cp), u32, vp, i32, i32, P(vp), P(u64)]
        L.spsp_tree_newick_host.restype = i32
        L.spsp_tree_newick_host.argtypes = [vp, u64, P(cp), u32, vp, i32, i32, P(vp), P(u64)]
        L.spsp_tree_files.restype = i32
        L.spsp_tree_files.argtypes = [vp, P(cp), u32, i32, i32, u32, u32, cp, i32, dbl, P(vp), P(u64)]
    if not LIB_OVERRIDDEN or hasattr(L, "spsp_keys_select_device"):
        L.spsp_keys_select_device.restype = i32
        L.spsp_keys_select_device.argtypes = [vp, u32, vp, vp, vp, vp, u32, u32, u32, u32, i32, P(vp), P(vp), P(vp), vp]
        L.spsp_select_band_host.restype = i32
        L.spsp_select_band_host.argtypes = [cp, u32, P(u32), P(u32)]
        L.spsp_sketch_from_keys_host.restype = i32
        L.spsp_sketch_from_keys_host.argtypes = [u32, u32, dbl, vp, vp, vp, u64, P(vp), P(u64)]
        L.spsp_select_files.restype = i32
        L.spsp_select_files.argtypes = [vp, P(cp), u32, u32, cp, i32, cp, i32, dbl, P(u64), P(u64)]
    if not LIB_OVERRIDDEN or hasattr(L, "spsp_accumulation_device"):
        L.spsp_accumulation_orders_host.restype = i32
        L.spsp_accumulation_orders_host.argtypes = [u32, u32, u64, vp]
        L.spsp_accumulation_plan_host.restype = i32
        L.spsp_accumulation_plan_host.argtypes = [u32, P(u32), P(u32), P(u32), P(u32)]
        L.spsp_accumulation_device.restype = i32
        L.spsp_accumulation_device.argtypes = [vp, u32, vp, vp, vp, vp, u32, vp, u32, vp, vp, vp]
        L.spsp_accumulation_csv_host.restype = i32
        L.spsp_accumulation_csv_host.argtypes = [vp, u32, u32, i32, P(vp), P(C.c_size_t)]
        L.spsp_accumulation_files.restype = i32
        L.spsp_accumulation_files.argtypes = [vp, P(cp), u32, u32, u64, i32, cp, i32, dbl, P(vp)]
    if not LIB_OVERRIDDEN or hasattr(L, "spsp_groups_device"):
        L.spsp_groups_labels_host.restype = i32
        L.spsp_groups_labels_host.argtypes = [vp, u64, u32, vp, P(u32), P(vp), P(u64)]
        L.spsp_groups_bounds_host.restype = i32
        L.spsp_groups_bounds_host.argtypes = [vp, u32, u32, u32, u32, u32, u32, vp, vp, vp]
        L.spsp_groups_device.restype = i32
        L.spsp_groups_device.argtypes = [vp, u32, vp, vp, vp, vp, u32, vp, u32, u32, u32, u32, u32, vp, vp, i32, P(vp), P(vp), P(vp), vp]
        L.spsp_groups_csv_host.restype = i32
        L.spsp_groups_csv_host.argtypes = [vp, u32, P(cp), i32, P(vp), P(u64)]
        L.spsp_groups_members_csv_host.restype = i32
        L.spsp_groups_members_csv_host.argtypes = [vp, u32, P(cp), vp, vp, vp, u32, P(cp), i32, P(vp), P(u64)]
        L.spsp_groups_files.restype = i32
        L.spsp_groups_files.argtypes = [vp, P(cp), u32, cp, i32, u32, u32, u32, u32, i32, cp, i32, dbl, P(vp), P(vp), P(u32)]
    if not LIB_OVERRIDDEN or hasattr(L, "spsp_classify_device"):
        L.spsp_classify_index_device.restype = i32
        L.spsp_classify_index_device.argtypes = [vp, u32, vp, vp, vp, vp, u32]
        L.spsp_classify_device.restype = i32
        L.spsp_classify_device.argtypes = [vp, vp, vp, vp, vp, u32, u32, u32, u32, u32, vp, vp]
        L.spsp_classify_plan_host.restype = i32
        L.spsp_classify_plan_host.argtypes = [u32, u32, P(u32), P(u32), P(u32), P(u32)]
        L.spsp_classify_csv_host.restype = i32
        L.spsp_classify_csv_host.argtypes = [vp, vp, u64, P(cp), P(cp), u32, u32, i32, P(vp), P(u64)]
        L.spsp_classify_summary_csv_host.restype = i32
        L.spsp_classify_summary_csv_host.argtypes = [vp, vp, u64, P(cp), u32, u32, P(vp), P(u64)]
        L.spsp_classify_stage_ms.restype = i32
        L.spsp_classify_stage_ms.argtypes = [vp, P(dbl)]
        L.spsp_classify_files.restype = i32
        L.spsp_classify_files.argtypes = [vp, P(cp), u32, cp, u32, u32, u32, u32, i32, cp, i32, dbl, P(vp), P(vp), P(u64)]
    if not LIB_OVERRIDDEN or hasattr(L, "spsp_depth_read_device"):
        L.spsp_depth_begin_device.restype = i32
        L.spsp_depth_begin_device.argtypes = [vp]
        L.spsp_depth_add_device.restype = i32
        L.spsp_depth_add_device.argtypes = [vp, vp, vp, vp, u64, u64]
        L.spsp_depth_read_device.restype = i32
        L.spsp_depth_read_device.argtypes = [vp, u32, vp, vp, P(vp)]
        L.spsp_depth_plan_host.restype = i32
        L.spsp_depth_plan_host.argtypes = [P(u32)]
        L.spsp_depth_stage_ms.restype = i32
        L.spsp_depth_stage_ms.argtypes = [vp, P(dbl)]
        L.spsp_depth_csv_host.restype = i32
        L.spsp_depth_csv_host.argtypes = [vp, P(cp), u32, i32, P(vp), P(u64)]
        L.spsp_depth_files.restype = i32
        L.spsp_depth_files.argtypes = [vp, P(cp), u32, P(cp), u32, u32, i32, cp, i32, dbl, P(vp), vp]
    if not LIB_OVERRIDDEN or hasattr(L, "spsp_profile_device"):
        L.spsp_profile_device.restype = i32
        L.spsp_profile_device.argtypes = [vp, u32, u32, u32, vp, P(u64), vp, P(vp)]
        L.spsp_profile_stage_ms.restype = i32
        L.spsp_profile_stage_ms.argtypes = [vp, P(dbl)]
        L.spsp_profile_counts.restype = i32
        L.spsp_profile_counts.argtypes = [vp, P(u32)]
        L.spsp_profile_csv_host.restype = i32
        L.spsp_profile_csv_host.argtypes = [vp, u64, vp, P(cp), u32, i32, P(vp), P(u64)]
        L.spsp_profile_files.restype = i32
        L.spsp_profile_files.argtypes = [vp, P(cp), u32, P(cp), u32, u32, u32, u32, i32, cp, i32, dbl, P(vp), vp, P(vp), P(u64), vp]
    if not LIB_OVERRIDDEN or hasattr(L, "spsp_taxonomy_device"):
        L.spsp_taxonomy_lineages_host.restype = i32
        L.spsp_taxonomy_lineages_host.argtypes = [cp, u64, u32, vp, P(vp), P(vp), P(vp), P(vp), P(u64), P(u32)]
        L.spsp_taxonomy_check_host.restype = i32
        L.spsp_taxonomy_check_host.argtypes = [vp, u32, vp, u32]
        L.spsp_taxonomy_plan_host.restype = i32
        L.spsp_taxonomy_plan_host.argtypes = [u32, P(u32), P(u32), P(u32), P(u32)]
        L.spsp_taxonomy_index_device.restype = i32
        L.spsp_taxonomy_index_device.argtypes = [vp, vp, u32, vp, u32, P(vp)]
        L.spsp_taxonomy_device.restype = i32
        L.spsp_taxonomy_device.argtypes = [vp, vp, vp, vp, vp, u32, u32, u32, u32, vp]
        L.spsp_taxonomy_stage_ms.restype = i32
        L.spsp_taxonomy_stage_ms.argtypes = [vp, P(dbl)]
        L.spsp_taxonomy_csv_host.restype = i32
        L.spsp_taxonomy_csv_host.argtypes = [vp, u64, P(cp), vp, u32, P(cp), i32, P(vp), P(u64)]
        L.spsp_taxonomy_report_csv_host.restype = i32
        L.spsp_taxonomy_report_csv_host.argtypes = [vp, u64, vp, u32, P(cp), vp, u32, P(vp), P(u64)]
        L.spsp_taxonomy_files.restype = i32
        L.spsp_taxonomy_files.argtypes = [vp, P(cp), u32, cp, cp, u32, u32, u32, i32, cp, i32, dbl, P(vp), P(u64)]
    if not LIB_OVERRIDDEN or hasattr(L, "spsp_records_extract_device"):
        L.spsp_extract_plan_host.restype = i32
        L.spsp_extract_plan_host.argtypes = [P(u32), P(u32)]
        L.spsp_records_extents_host.restype = i32
        L.spsp_records_extents_host.argtypes = [vp, u64, P(vp), P(u32)]
        L.spsp_records_extract_host.restype = i32
        L.spsp_records_extract_host.argtypes = [vp, u64, vp, u32, vp, P(vp), P(u64), P(u64)]
        L.spsp_extract_flags_classify_host.restype = i32
        L.spsp_extract_flags_classify_host.argtypes = [cp, vp, vp, u64, u32, u32, vp]
        L.spsp_extract_flags_taxonomy_host.restype = i32
        L.spsp_extract_flags_taxonomy_host.argtypes = [cp, vp, u64, vp, u32, vp]
        L.spsp_extract_word_check_host.restype = i32
        L.spsp_extract_word_check_host.argtypes = [cp, i32, u32]
        L.spsp_records_extents_device.restype = i32
        L.spsp_records_extents_device.argtypes = [vp, vp, u64, P(vp), P(u32)]
        L.spsp_records_extract_device.restype = i32
        L.spsp_records_extract_device.argtypes = [vp, vp, u64, vp, u32, vp, P(vp), P(u64), P(u64)]
        L.spsp_extract_stage_ms.restype = i32
        L.spsp_extract_stage_ms.argtypes = [vp, P(dbl)]
        L.spsp_classify_files_extract.restype = i32
        L.spsp_classify_files_extract.argtypes = [vp, P(cp), u32, cp, u32, u32, u32, u32, i32, cp, i32, dbl, P(vp), P(vp), P(u64), cp, i32, P(u64), P(u64)]
        L.spsp_taxonomy_files_extract.restype = i32
        L.spsp_taxonomy_files_extract.argtypes = [vp, P(cp), u32, cp, cp, u32, u32, u32, i32, cp, i32, dbl, P(vp), P(u64), cp, i32, P(u64), P(u64)]
    if not LIB_OVERRIDDEN or hasattr(L, "spsp_records_split_device"):
        L.spsp_split_plan_host.restype = i32
        L.spsp_split_plan_host.argtypes = [P(u32), P(u32), P(u32), P(u32)]
        L.spsp_records_split_host.restype = i32
        L.spsp_records_split_host.argtypes = [vp, u64, vp, u32, vp, u32, P(vp), P(u64), P(vp), P(vp)]
        L.spsp_split_bins_classify_host.restype = i32
        L.spsp_split_bins_classify_host.argtypes = [cp, vp, vp, u64, u32, u32, vp, P(u32)]
        L.spsp_split_bins_taxonomy_host.restype = i32
        L.spsp_split_bins_taxonomy_host.argtypes = [cp, vp, u64, vp, vp, u32, vp, P(u32)]
        L.spsp_split_word_check_host.restype = i32
        L.spsp_split_word_check_host.argtypes = [cp, i32]
        L.spsp_split_csv_host.restype = i32
        L.spsp_split_csv_host.argtypes = [cp, P(cp), cp, u32, vp, vp, cp, vp, cp, P(vp), P(u64)]
        L.spsp_records_split_device.restype = i32
        L.spsp_records_split_device.argtypes = [vp, vp, u64, vp, u32, vp, u32, P(vp), P(u64), vp, vp]
        L.spsp_split_stage_ms.restype = i32
        L.spsp_split_stage_ms.argtypes = [vp, P(dbl)]
        L.spsp_classify_files_split.restype = i32
        L.spsp_classify_files_split.argtypes = [vp, P(cp), u32, cp, cp, u32, u32, u32, u32, i32, cp, i32, dbl, cp, i32, P(vp), P(vp), P(u64), P(u64), P(u64)]
        L.spsp_taxonomy_files_split.restype = i32
        L.spsp_taxonomy_files_split.argtypes = [vp, P(cp), u32, cp, cp, cp, u32, u32, u32, i32, cp, i32, dbl, cp, i32, P(vp), P(u64), P(u64), P(u64)]
    if not LIB_OVERRIDDEN or hasattr(L, "spsp_records_union_device"):
        L.spsp_pairs_names_host.restype = i32
        L.spsp_pairs_names_host.argtypes = [P(cp), P(cp), u64, P(vp), P(u64)]
        L.spsp_union_plan_host.restype = i32
        L.spsp_union_plan_host.argtypes = [P(u32), P(u32)]
        L.spsp_records_union_device.restype = i32
        L.spsp_records_union_device.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, u32, P(vp), P(vp), P(vp), vp]
        L.spsp_union_stage_ms.restype = i32
        L.spsp_union_stage_ms.argtypes = [vp, P(dbl)]
        L.spsp_classify_files_paired.restype = i32
        L.spsp_classify_files_paired.argtypes = [vp, P(cp), u32, cp, cp, u32, u32, u32, u32, i32, cp, i32, dbl, cp, i32, P(vp), P(vp), P(u64), P(u64), P(u64)]
        L.spsp_taxonomy_files_paired.restype = i32
        L.spsp_taxonomy_files_paired.argtypes = [vp, P(cp), u32, cp, cp, cp, u32, u32, u32, i32, cp, i32, dbl, cp, i32, P(vp), P(u64), P(u64), P(u64)]
    if not LIB_OVERRIDDEN or hasattr(L, "spsp_records_windows_device"):
        L.spsp_windows_plan_host.restype = i32
        L.spsp_windows_plan_host.argtypes = [P(u32), P(u32), P(u32)]
        L.spsp_records_windows_host.restype = i32
        L.spsp_records_windows_host.argtypes = [vp, u32, u32, u64, vp, P(vp), P(u64), P(u64)]
        L.spsp_windows_expand_host.restype = i32
        L.spsp_windows_expand_host.argtypes = [vp, vp, u32, u32, u64, P(vp), P(u64), vp, P(vp), P(u64)]
        L.spsp_windows_segments_host.restype = i32
        L.spsp_windows_segments_host.argtypes = [vp, vp, vp, vp, vp, vp, u32, u32, u64, u32, P(vp), P(u64), vp]
        L.spsp_segments_csv_host.restype = i32
        L.spsp_segments_csv_host.argtypes = [vp, u64, P(cp), u32, P(cp), cp, u32, P(vp), P(u64)]
        L.spsp_mosaic_csv_host.restype = i32
        L.spsp_mosaic_csv_host.argtypes = [vp, u32, P(cp), P(cp), cp, u32, i32, P(vp), P(u64)]
        L.spsp_windows_word_check_host.restype = i32
        L.spsp_windows_word_check_host.argtypes = [cp, i32]
        L.spsp_records_windows_device.restype = i32
        L.spsp_records_windows_device.argtypes = [vp, vp, u64, vp, u32, u32, u64, i32, P(vp), P(u64), P(vp), vp, P(u64)]
        L.spsp_windows_stage_ms.restype = i32
        L.spsp_windows_stage_ms.argtypes = [vp, P(dbl)]
        L.spsp_classify_files_windows.restype = i32
        L.spsp_classify_files_windows.argtypes = [vp, P(cp), u32, cp, u32, u32, u32, u32, i32, cp, i32, dbl, u64, cp, P(vp), P(vp), P(u64), P(vp), P(u64), P(vp),
                                                  P(u64), P(vp)]
        L.spsp_taxonomy_files_windows.restype = i32
        L.spsp_taxonomy_files_windows.argtypes = [vp, P(cp), u32, cp, cp, u32, u32, u32, i32, cp, i32, dbl, u64, cp, P(vp), P(u64), P(vp), P(u64), P(vp), P(u64), P(vp)]
    if not LIB_OVERRIDDEN or hasattr(L, "spsp_segments_write_device"):
        L.spsp_segments_plan_host.restype = i32
        L.spsp_segments_plan_host.argtypes = [P(u32), P(u32)]
        L.spsp_windows_smooth_host.restype = i32
        L.spsp_windows_smooth_host.argtypes = [vp, vp, vp, u32, u32, u32, P(u64)]
        L.spsp_segments_word_check_host.restype = i32
        L.spsp_segments_word_check_host.argtypes = [cp, i32, u32]
        L.spsp_segments_select_host.restype = i32
        L.spsp_segments_select_host.argtypes = [vp, u64, vp, u32, u32, cp, u64, vp, P(u64), P(u64)]
        L.spsp_segments_fasta_host.restype = i32
        L.spsp_segments_fasta_host.argtypes = [vp, u64, vp, u32, vp, u64, vp, P(cp), P(cp), cp, u32, P(vp), P(u64)]
        L.spsp_segments_write_device.restype = i32
        L.spsp_segments_write_device.argtypes = [vp, vp, u64, i32, vp, vp, vp, vp, u64, P(vp), P(u64)]
        L.spsp_segments_stage_ms.restype = i32
        L.spsp_segments_stage_ms.argtypes = [vp, P(dbl)]
        tail = [u32, cp, u64, i32, P(u64), P(u64), P(u64)]
        L.spsp_classify_files_segments.restype = i32
        L.spsp_classify_files_segments.argtypes = L.spsp_classify_files_windows.argtypes + tail
        L.spsp_taxonomy_files_segments.restype = i32
        L.spsp_taxonomy_files_segments.argtypes = L.spsp_taxonomy_files_windows.argtypes + tail
    if not LIB_OVERRIDDEN or hasattr(L, "spsp_records_lift_device"):
        L.spsp_lift_plan_host.restype = i32
        L.spsp_lift_plan_host.argtypes = [P(u32), P(u32)]
        L.spsp_records_lift_host.restype = i32
        L.spsp_records_lift_host.argtypes = [vp, u64, vp, u64, vp, vp, vp, P(u32)]
        L.spsp_segments_bed_host.restype = i32
        L.spsp_segments_bed_host.argtypes = [vp, u64, vp, vp, P(cp), u32, P(cp), cp, u32, P(vp), P(u64)]
        L.spsp_records_lift_device.restype = i32
        L.spsp_records_lift_device.argtypes = [vp, vp, u64, u64, vp, u64, vp, vp, vp, P(u32)]
        L.spsp_lift_stage_ms.restype = i32
        L.spsp_lift_stage_ms.argtypes = [vp, P(dbl)]
        raw_tail = [i32, P(vp), P(vp), P(u64)]
        L.spsp_classify_files_raw.restype = i32
        L.spsp_classify_files_raw.argtypes = L.spsp_classify_files_segments.argtypes + raw_tail
        L.spsp_taxonomy_files_raw.restype = i32
        L.spsp_taxonomy_files_raw.argtypes = L.spsp_taxonomy_files_segments.argtypes + raw_tail
    _lib = L
    return L


def library_info():
    """which shared library this process computes with (path, version string, whether SPSP_LIB replaced the in-tree build)"""
    return {"path": os.path.relpath(LIB_PATH, os.path.dirname(_HERE)) if not LIB_OVERRIDDEN else LIB_PATH,
            "version": lib().spsp_version().decode(), "overridden_by_SPSP_LIB": LIB_OVERRIDDEN}


def _check(rc):
    if rc != 0:
        e = SpspError("libspsp error %d: %s" % (rc, lib().spsp_last_error().decode(errors="replace")))
        e.code = rc
        raise e


def _take(ptr, nbytes):
    data = C.string_at(ptr, nbytes) if nbytes else b""
    lib().spsp_free(ptr)
    return data


def slot_bytes(n, slot_cap, k):
    return int(lib().spsp_slot_bytes(n, slot_cap, k))


def threshold(k, m, s):
    """selection threshold for -s (Subsampler::compute_threshold)."""
    return lib().spsp_threshold_host(k, m, float(s))


def make_params(k=31, m=11, s=1000.0, abundance=1, flags=SPSP_SCAN_DEFAULT, threshold_value=None):
    p = Params()
    p.k, p.m, p.abundance, p.flags = k, m, abundance, flags
    p.threshold = threshold(k, m, s) if threshold_value is None else threshold_value
    return p


def clean_fasta(text):
    """FASTA bytes (already gunzipped) -> (bases uint8[n], rec_off uint64[n_rec+1])."""
    bases, offs, n_rec = C.c_void_p(), C.c_void_p(), C.c_uint32()
    _check(lib().spsp_fasta_clean_host(text, len(text), C.byref(bases), C.byref(offs), C.byref(n_rec)))
    off = np.frombuffer(_take(offs, 8 * (n_rec.value + 1)), dtype=np.uint64).copy()
    b = np.frombuffer(_take(bases, int(off[-1])), dtype=np.uint8).copy()
    return b, off


def sketch_build(params, rate, bases, rec_off, superkmers):
    """super-k-mer stream -> (uncompressed sketch payload, stats dict)."""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    rec_off = np.ascontiguousarray(rec_off, dtype=np.uint64)
    sk = np.ascontiguousarray(superkmers, dtype=SUPERKMER_DTYPE)
    out, n, st = C.c_void_p(), C.c_uint64(), SketchStats()
    _check(lib().spsp_sketch_build_host(C.byref(params), float(rate), bases.ctypes.data, rec_off.ctypes.data,
                                        len(rec_off) - 1, sk.ctypes.data, len(sk), C.byref(out), C.byref(n),
                                        C.byref(st)))
    return _take(out, n.value), {f: getattr(st, f) for f, _ in SketchStats._fields_}


class Sketch:
    """Parsed sketch: sorted distinct (minimizer, canonical k-mer) keys."""

    def __init__(self, k, m, minimizer, kmer_lo, kmer_hi):
        self.k, self.m = k, m
        self.minimizer, self.kmer_lo, self.kmer_hi = minimizer, kmer_lo, kmer_hi

    def __len__(self):
        return len(self.minimizer)

    def key_set(self):
        return {(int(a), (int(h) << 64) | int(l)) for a, l, h in zip(self.minimizer, self.kmer_lo, self.kmer_hi)}


def sketch_parse(payload):
    k, m, n = C.c_uint32(), C.c_uint32(), C.c_uint64()
    mn, lo, hi = C.c_void_p(), C.c_void_p(), C.c_void_p()
    _check(lib().spsp_sketch_parse_host(payload, len(payload), C.byref(k), C.byref(m), C.byref(mn), C.byref(lo),
                                        C.byref(hi), C.byref(n)))
    c = n.value
    a = np.frombuffer(_take(mn, 4 * c), dtype=np.uint32).copy()
    b = np.frombuffer(_take(lo, 8 * c), dtype=np.uint64).copy()
    d = np.frombuffer(_take(hi, 8 * c), dtype=np.uint64).copy()
    return Sketch(k.value, m.value, a, b, d)


def sketch_header(payload):
    """header line of a gunzipped sketch payload -> (k, m, k-mer count, sampling rate)"""
    k, m, n, r = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_double()
    _check(lib().spsp_sketch_header_host(payload, len(payload), C.byref(k), C.byref(m), C.byref(n), C.byref(r)))
    return k.value, m.value, n.value, r.value


def sketch_downsample(payload, rate):
    """a sketch payload brought down to the coarser sampling rate `rate` (spsp_sketch_downsample_host): the buckets whose
    minimizer passes, as they are, behind a header that names `rate` and the distinct keys left"""
    out, n = C.c_void_p(), C.c_uint64()
    _check(lib().spsp_sketch_downsample_host(payload, len(payload), float(rate), C.byref(out), C.byref(n)))
    return _take(out, n.value)


def sketch_from_keys(k, m, rate, mn, lo, hi=None):
    """spsp_sketch_from_keys_host: sorted distinct keys (minimizer, kmer_lo[, kmer_hi for k > 32]) -> an uncompressed sketch payload
    that sketch_parse reads back as exactly those keys: one non-maximal super-k-mer of k bases per key"""
    mn = np.ascontiguousarray(mn, dtype=np.uint32)
    lo = np.ascontiguousarray(lo, dtype=np.uint64)
    if len(lo) != len(mn) or (hi is not None and len(hi) != len(mn)):
        raise ValueError("sketch_from_keys: one kmer_lo (and kmer_hi) per minimizer")
    if hi is not None:
        hi = np.ascontiguousarray(hi, dtype=np.uint64)
    out, n = C.c_void_p(), C.c_uint64()
    _check(lib().spsp_sketch_from_keys_host(k, m, float(rate), mn.ctypes.data, lo.ctypes.data, hi.ctypes.data if hi is not None else None,
                                            len(mn), C.byref(out), C.byref(n)))
    return _take(out, n.value)


def select_band(what, R):
    """spsp_select_band_host: a band word (union, present, absent, all, core=<t>, unique=<t>, shell=<t>, <a>..<b>) among R
    references -> (h_min, h_max); an empty band is (1, 0)"""
    a, b = C.c_uint32(), C.c_uint32()
    _check(lib().spsp_select_band_host(str(what).encode(), R, C.byref(a), C.byref(b)))
    return a.value, b.value


def _rate_arg(rate):
    """rate keyword of the comparator drivers: 0.0 (the headers' rates ignored), a rate, or "auto" (the coarsest of the files')"""
    if isinstance(rate, str):
        if rate != "auto":
            raise ValueError("rate: a number or \"auto\", not %r" % rate)
        return RATE_COARSEST
    return float(rate)


def csv(jaccard, names, inter, card, n_query=None, precision=6, min_threshold=0.0):
    n = len(names)
    nq = n if n_query is None else n_query
    inter = np.ascontiguousarray(inter, dtype=np.uint32)
    card = np.ascontiguousarray(card, dtype=np.uint64)
    arr = (C.c_char_p * n)(*[s.encode() for s in names])
    out, ln = C.c_void_p(), C.c_uint64()
    _check(lib().spsp_csv_host(1 if jaccard else 0, arr, n, nq, inter.ctypes.data, card.ctypes.data, precision,
                               float(min_threshold), C.byref(out), C.byref(ln)))
    return _take(out, ln.value)


def csv_cells(jaccard, names, cells, card, n_query=None, precision=6, min_threshold=0.0):
    """the printers from the sparse form of the pair matrix: cells = uint64 array of i << 48 | j << 32 | count (i < j)"""
    n = len(names)
    nq = n if n_query is None else n_query
    cells = np.ascontiguousarray(cells, dtype=np.uint64)
    card = np.ascontiguousarray(card, dtype=np.uint64)
    arr = (C.c_char_p * n)(*[s.encode() for s in names])
    out, ln = C.c_void_p(), C.c_uint64()
    _check(lib().spsp_csv_cells_host(1 if jaccard else 0, arr, n, nq, cells.ctypes.data, len(cells), card.ctypes.data, precision,
                                     float(min_threshold), C.byref(out), C.byref(ln)))
    return _take(out, ln.value)


def csv_cells_gz(jaccard, names, cells, card, gz_path, n_query=None, precision=6, min_threshold=0.0):
    """spsp_csv_cells_gz_host: the same matrix straight into a .csv.gz (gzip members made without the text in between)"""
    n = len(names)
    nq = n if n_query is None else n_query
    cells = np.ascontiguousarray(cells, dtype=np.uint64)
    card = np.ascontiguousarray(card, dtype=np.uint64)
    arr = (C.c_char_p * n)(*[s.encode() for s in names])
    _check(lib().spsp_csv_cells_gz_host(1 if jaccard else 0, arr, n, nq, cells.ctypes.data, len(cells), card.ctypes.data, precision,
                                        float(min_threshold), gz_path.encode()))


def gather_csv(rows, names, card, n_query, precision=6):
    """spsp_gather_csv_host: gather rows (GATHER_ROW_DTYPE array) -> the text of <prefix>_gather.csv.gz; card[i] = key count of
    sketch i as the gather saw it, names = the n_query queries' names, then the references'"""
    rows = np.ascontiguousarray(rows, dtype=GATHER_ROW_DTYPE)
    card = np.ascontiguousarray(card, dtype=np.uint64)
    n = len(names)
    arr = (C.c_char_p * n)(*[s.encode() for s in names])
    out, ln = C.c_void_p(), C.c_uint64()
    _check(lib().spsp_gather_csv_host(rows.ctypes.data, len(rows), arr, n, n_query, card.ctypes.data, precision, C.byref(out), C.byref(ln)))
    return _take(out, ln.value)


def cluster_csv(rows, names, card, metric, precision=6):
    """spsp_cluster_csv_host: cluster rows (CLUSTER_ROW_DTYPE array, one per sketch in list order) -> the text of
    <prefix>_clusters.csv.gz; card[i] = key count of sketch i as the clustering saw it"""
    rows = np.ascontiguousarray(rows, dtype=CLUSTER_ROW_DTYPE)
    card = np.ascontiguousarray(card, dtype=np.uint64)
    n = len(names)
    if len(rows) != n or len(card) != n:
        raise ValueError("cluster_csv: one row and one key count per name")
    arr = (C.c_char_p * n)(*[s.encode() for s in names])
    out, ln = C.c_void_p(), C.c_uint64()
    _check(lib().spsp_cluster_csv_host(rows.ctypes.data, arr, n, card.ctypes.data, metric, precision, C.byref(out), C.byref(ln)))
    return _take(out, ln.value)


def tree_cut(rows, card, metric, floor_num, floor_den, num, den):
    """spsp_tree_cut_host: the rows of a linkage tree built at the floor floor_num / floor_den (TREE_ROW_DTYPE array), cut at
    num / den (not below the floor) -> (cluster: np.uint32 per sketch, numbered by first-listed member, n_clusters): what
    cluster_cells_device reports at num / den on the same cells"""
    rows = np.ascontiguousarray(rows, dtype=TREE_ROW_DTYPE)
    card = np.ascontiguousarray(card, dtype=np.uint64)
    n = len(card)
    cluster = np.zeros(n, dtype=np.uint32)
    nc = C.c_uint64()
    _check(lib().spsp_tree_cut_host(rows.ctypes.data, len(rows), n, card.ctypes.data, metric, floor_num, floor_den, num, den, cluster.ctypes.data, C.byref(nc)))
    return cluster, nc.value


def _tree_text(call, what, rows, names, card, metric, precision):
    rows = np.ascontiguousarray(rows, dtype=TREE_ROW_DTYPE)
    card = np.ascontiguousarray(card, dtype=np.uint64)
    n = len(names)
    if len(card) != n:
        raise ValueError("%s: one key count per name" % what)
    arr = (C.c_char_p * n)(*[s.encode() for s in names])
    out, ln = C.c_void_p(), C.c_uint64()
    _check(call(rows.ctypes.data, len(rows), arr, n, card.ctypes.data, metric, precision, C.byref(out), C.byref(ln)))
    return _take(out, ln.value)


def tree_csv(rows, names, card, metric, precision=6):
    """spsp_tree_csv_host: linkage-tree rows (TREE_ROW_DTYPE array, best merge first) -> the text of <prefix>_tree.csv.gz;
    card[i] = key count of sketch i as the comparison saw it"""
    return _tree_text(lib().spsp_tree_csv_host, "tree_csv", rows, names, card, metric, precision)


def tree_newick(rows, names, card, metric, precision=6):
    """spsp_tree_newick_host: linkage-tree rows -> the text of <prefix>_tree.nwk: one Newick tree, quoted names, node height
    1 - score, what never merged joined at height 1"""
    return _tree_text(lib().spsp_tree_newick_host, "tree_newick", rows, names, card, metric, precision)


def neighbours_csv(rows, passing, names, card, metric, n_query=None, precision=6):
    """spsp_neighbours_csv_host: neighbour rows (NEIGHBOUR_ROW_DTYPE array) and the per-row passing counts -> the text of
    <prefix>_neighbours.csv.gz; card[i] = key count of sketch i as the comparison saw it, names = the queries' names first in
    query mode (n_query < len(names))"""
    rows = np.ascontiguousarray(rows, dtype=NEIGHBOUR_ROW_DTYPE)
    card = np.ascontiguousarray(card, dtype=np.uint64)
    n = len(names)
    nq = n if n_query is None else n_query
    if len(card) != n:
        raise ValueError("neighbours_csv: one key count per name")
    if passing is not None:
        passing = np.ascontiguousarray(passing, dtype=np.uint32)
        if len(passing) != min(n, nq):
            raise ValueError("neighbours_csv: one passing count per row sketch")
    arr = (C.c_char_p * n)(*[s.encode() for s in names])
    out, ln = C.c_void_p(), C.c_uint64()
    _check(lib().spsp_neighbours_csv_host(rows.ctypes.data, len(rows), passing.ctypes.data if passing is not None else None, arr, n, nq,
                                          card.ctypes.data, metric, precision, C.byref(out), C.byref(ln)))
    return _take(out, ln.value)


def prevalence_csv(rows, names, card, precision=6):
    """spsp_prevalence_csv_host: prevalence rows (PREVALENCE_ROW_DTYPE array, one per row sketch in list order) -> the text of
    <prefix>_prevalence.csv.gz; names[i], card[i] = the name and the key count of row sketch i as the prevalence pass saw it"""
    rows = np.ascontiguousarray(rows, dtype=PREVALENCE_ROW_DTYPE)
    card = np.ascontiguousarray(card, dtype=np.uint64)
    n = len(rows)
    if len(names) < n or len(card) < n:
        raise ValueError("prevalence_csv: a name and a key count per row")
    arr = (C.c_char_p * max(n, 1))(*[s.encode() for s in names[:n]])
    out, ln = C.c_void_p(), C.c_uint64()
    _check(lib().spsp_prevalence_csv_host(rows.ctypes.data, n, arr, card.ctypes.data, precision, C.byref(out), C.byref(ln)))
    return _take(out, ln.value)


def spectrum_csv(spectrum):
    """spsp_spectrum_csv_host: spectrum[t] = the distinct keys held by exactly t references, t = 0 .. R ([0] ignored) -> the text
    of <prefix>_spectrum.csv.gz"""
    spectrum = np.ascontiguousarray(spectrum, dtype=np.uint64)
    if len(spectrum) < 1:
        raise ValueError("spectrum_csv: R + 1 words")
    out, ln = C.c_void_p(), C.c_uint64()
    _check(lib().spsp_spectrum_csv_host(spectrum.ctypes.data, len(spectrum) - 1, C.byref(out), C.byref(ln)))
    return _take(out, ln.value)


def accumulation_orders(n, n_orders, seed):
    """spsp_accumulation_orders_host: the orders a seed names -> np.uint32[n_orders, n]; order 0 is the list order, the others are
    Fisher-Yates shuffles drawn from one splitmix64 stream (include/spsp.h spells the rule out)"""
    out = np.zeros((max(n_orders, 0), max(n, 0)), dtype=np.uint32)
    _check(lib().spsp_accumulation_orders_host(n, n_orders, seed, out.ctypes.data if out.size else None))
    return out


def accumulation_plan(n):
    """spsp_accumulation_plan_host: what the device call runs with for n sketches -> dict(group: orders per pass over the keys,
    window: ranks per window of the first-rank histogram, bitmap_bits: ranks per mex pass of a long list, cut: the list length
    above which the whole wave walks a list)"""
    g, w, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    _check(lib().spsp_accumulation_plan_host(n, C.byref(g), C.byref(w), C.byref(b), C.byref(c)))
    return {"group": g.value, "window": w.value, "bitmap_bits": b.value, "cut": c.value}


def accumulation_csv(rows, n_orders, precision=6):
    """spsp_accumulation_csv_host: accumulation rows (ACCUMULATION_ROW_DTYPE array, row j-1 is step j) over n_orders orders -> the
    text of <prefix>_accumulation.csv.gz"""
    rows = np.ascontiguousarray(rows, dtype=ACCUMULATION_ROW_DTYPE)
    out, ln = C.c_void_p(), C.c_size_t()
    _check(lib().spsp_accumulation_csv_host(rows.ctypes.data if len(rows) else None, len(rows), n_orders, precision, C.byref(out), C.byref(ln)))
    return _take(out, ln.value)


def classify_plan(n_ref, top=1):
    """spsp_classify_plan_host: what routes a record for n_ref references -> dict(small_work: the work (sum of its keys' holders) up
    to which one wave tallies a record in LDS, lds_refs: the references up to which the workgroup form keeps its counters in LDS,
    counters_in_lds: whether they do for n_ref, list_cut: the holders above which a whole wave walks a key's list)"""
    a, b, c, d = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    _check(lib().spsp_classify_plan_host(n_ref, top, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
    return {"small_work": a.value, "lds_refs": b.value, "counters_in_lds": bool(c.value), "list_cut": d.value}


def depth_plan():
    """spsp_depth_plan_host: the bins of one LDS histogram of the depth reduction; the last bin holds every count at or above bins - 1"""
    bins = C.c_uint32()
    _check(lib().spsp_depth_plan_host(C.byref(bins)))
    return bins.value


def depth_csv(rows, names, precision=6):
    """spsp_depth_csv_host: rows (DEPTH_ROW_DTYPE, one per reference) and the references' names -> the text of <prefix>_depth.csv.gz"""
    rows = np.ascontiguousarray(rows, dtype=DEPTH_ROW_DTYPE)
    if len(names) != len(rows):
        raise ValueError("depth_csv: one name per row")
    arr, _alive = _paths_array(names)
    text, n = C.c_void_p(), C.c_uint64()
    _check(lib().spsp_depth_csv_host(rows.ctypes.data if len(rows) else None, arr, len(rows), precision, C.byref(text), C.byref(n)))
    return _take(text, n.value)


def profile_csv(rows, totals, names, precision=6):
    """spsp_profile_csv_host: rows (PROFILE_ROW_DTYPE, one per round), the call's totals (a PROFILE_TOTALS_DTYPE scalar) and the names
    of ALL references of the index -> the text of <prefix>_profile.csv.gz"""
    rows = np.ascontiguousarray(rows, dtype=PROFILE_ROW_DTYPE)
    totals = np.ascontiguousarray(totals, dtype=PROFILE_TOTALS_DTYPE).reshape(1)
    arr, _alive = _paths_array(names)
    text, n = C.c_void_p(), C.c_uint64()
    _check(lib().spsp_profile_csv_host(rows.ctypes.data if len(rows) else None, len(rows), totals.ctypes.data, arr, len(names), precision, C.byref(text), C.byref(n)))
    return _take(text, n.value)


def _classify_rows(records, hits, top):
    records = np.ascontiguousarray(records, dtype=CLASSIFY_RECORD_DTYPE)
    hits = np.ascontiguousarray(hits, dtype=CLASSIFY_HIT_DTYPE).reshape(-1)
    if len(hits) != len(records) * top:
        raise ValueError("classification rows: `top` hits per record")
    return records, hits


def classify_csv(records, hits, record_names, ref_names, top, precision=6):
    """spsp_classify_csv_host: records (CLASSIFY_RECORD_DTYPE), their hits (CLASSIFY_HIT_DTYPE, `top` per record), the records' and
    the references' names -> the text of <prefix>_classify.csv.gz"""
    records, hits = _classify_rows(records, hits, top)
    if len(record_names) != len(records):
        raise ValueError("classify_csv: one name per record")
    r_arr, _a = _paths_array(record_names)
    f_arr, _b = _paths_array(ref_names)
    out, ln = C.c_void_p(), C.c_uint64()
    _check(lib().spsp_classify_csv_host(records.ctypes.data if len(records) else None, hits.ctypes.data if len(hits) else None, len(records), r_arr, f_arr,
                                        len(ref_names), top, precision, C.byref(out), C.byref(ln)))
    return _take(out, ln.value)


def classify_summary_csv(records, hits, ref_names, top):
    """spsp_classify_summary_csv_host: the same rows -> the text of <prefix>_classify_summary.csv.gz"""
    records, hits = _classify_rows(records, hits, top)
    f_arr, _b = _paths_array(ref_names)
    out, ln = C.c_void_p(), C.c_uint64()
    _check(lib().spsp_classify_summary_csv_host(records.ctypes.data if len(records) else None, hits.ctypes.data if len(hits) else None, len(records), f_arr,
                                                len(ref_names), top, C.byref(out), C.byref(ln)))
    return _take(out, ln.value)


def taxonomy_lineages(text, n_ref):
    """spsp_taxonomy_lineages_host: the text of a lineage file (one name;name;... line per reference, in list order) for n_ref
    references -> dict(parent, depth, size: np.uint32[T] in preorder, ref_node: np.uint32[n_ref], names: the T names, node 0 is
    "root")"""
    if isinstance(text, str):
        text = text.encode()
    ref_node = np.zeros(max(n_ref, 1), dtype=np.uint32)
    parent, depth, size, names, ln, T = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint32()
    _check(lib().spsp_taxonomy_lineages_host(text, len(text), n_ref, ref_node.ctypes.data, C.byref(parent), C.byref(depth), C.byref(size), C.byref(names),
                                             C.byref(ln), C.byref(T)))
    arrays = [np.frombuffer(_take(p, T.value * 4), dtype=np.uint32).copy() for p in (parent, depth, size)]
    blob = _take(names, ln.value)
    return {"parent": arrays[0], "depth": arrays[1], "size": arrays[2], "ref_node": ref_node[:n_ref], "names": [x.decode() for x in blob.split(b"\0")[:T.value]]}


def taxonomy_check(parent, ref_node):
    """spsp_taxonomy_check_host: raises SpspError(ERR_ARG) unless parent is a tree of 1 .. 1 048 576 nodes numbered in preorder, no
    deeper than 32, and every ref_node names one of its nodes"""
    parent = np.ascontiguousarray(parent, dtype=np.uint32)
    ref_node = np.ascontiguousarray(ref_node, dtype=np.uint32)
    _check(lib().spsp_taxonomy_check_host(parent.ctypes.data if len(parent) else None, len(parent), ref_node.ctypes.data if len(ref_node) else None, len(ref_node)))


def taxonomy_plan(n_nodes):
    """spsp_taxonomy_plan_host: the cuts of the two forms for a tree of n_nodes -> dict(small_hits: the hit keys up to which one wave
    sorts a record's nodes in LDS, lds_nodes: the nodes up to which the workgroup form keeps its counters in LDS, counters_in_lds:
    whether they do for n_nodes, list_cut: the holders above which a whole wave folds a key's list when the taxonomy is attached)"""
    a, b, c, d = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    _check(lib().spsp_taxonomy_plan_host(n_nodes, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
    return {"small_hits": a.value, "lds_nodes": b.value, "counters_in_lds": bool(c.value), "list_cut": d.value}


def union_plan():
    """spsp_union_plan_host: the constants the union's kernels cut at -> dict(threads: the lanes of a workgroup, a lane per key;
    tile: the entries of side B per count of the scan)"""
    a, b = C.c_uint32(), C.c_uint32()
    _check(lib().spsp_union_plan_host(C.byref(a), C.byref(b)))
    return {"threads": a.value, "tile": b.value}


def pairs_names(names1, names2):
    """spsp_pairs_names_host: the naming rule of paired records (include/spsp.h) over two lists of first words -> the common
    names (bytes).  Lists of different lengths raise ValueError; the first pair whose names differ raises SpspError
    (SPSP_ERR_FORMAT) with that pair's number as its .bad"""
    if len(names1) != len(names2):
        raise ValueError("pairs_names: one name per mate")
    n = len(names1)
    enc = [[x if isinstance(x, bytes) else str(x).encode() for x in names] for names in (names1, names2)]
    a1, a2 = (C.c_char_p * max(n, 1))(*enc[0]), (C.c_char_p * max(n, 1))(*enc[1])
    common, bad = C.c_void_p(), C.c_uint64()
    rc = lib().spsp_pairs_names_host(a1, a2, n, C.byref(common), C.byref(bad))
    if rc != 0:
        try:
            _check(rc)
        except SpspError as e:
            e.bad = bad.value
            raise
    size = sum(len(x) - (2 if x.endswith(b"/1") else 0) + 1 for x in enc[0])
    blob = _take(common, size)
    return bytes(blob).split(b"\0")[:n] if n else []


def extract_plan():
    """spsp_extract_plan_host: the two constants the extraction's kernels cut at -> dict(tile_bytes: the bytes of the text one
    workgroup of the starts pass reads, stretch_bytes: the bytes of the output one workgroup of the copy owns)"""
    a, b = C.c_uint32(), C.c_uint32()
    _check(lib().spsp_extract_plan_host(C.byref(a), C.byref(b)))
    return {"tile_bytes": a.value, "stretch_bytes": b.value}


def records_extents(text):
    """spsp_records_extents_host: the bytes of a FASTA / FASTQ text (FASTQ: the first byte is '@') -> begin: np.uint64[n_rec + 1];
    record r is text[begin[r]:begin[r + 1]] (the rule: include/spsp.h, "extract")"""
    text = np.frombuffer(bytes(text), dtype=np.uint8)
    out, n = C.c_void_p(), C.c_uint32()
    _check(lib().spsp_records_extents_host(text.ctypes.data if len(text) else None, len(text), C.byref(out), C.byref(n)))
    return np.frombuffer(_take(out, (n.value + 1) * 8), dtype=np.uint64).copy()


def records_extract(text, keep, begin=None):
    """spsp_records_extract_host: the records of `text` with keep[r] != 0, back to back, a newline appended to a last record that
    lacks one -> (bytes, n_kept).  begin: the records' starts (records_extents(text) when None)"""
    if begin is None:
        begin = records_extents(text)
    text = np.frombuffer(bytes(text), dtype=np.uint8)
    begin = np.ascontiguousarray(begin, dtype=np.uint64)
    keep = np.ascontiguousarray(keep, dtype=np.uint8)
    if len(begin) < 1 or len(keep) != len(begin) - 1:
        raise ValueError("records_extract: one flag per record and n_rec + 1 starts")
    out, n_out, n_kept = C.c_void_p(), C.c_uint64(), C.c_uint64()
    _check(lib().spsp_records_extract_host(text.ctypes.data if len(text) else None, len(text), begin.ctypes.data, len(keep), keep.ctypes.data if len(keep) else None,
                                           C.byref(out), C.byref(n_out), C.byref(n_kept)))
    return _take(out, n_out.value), n_kept.value


def extract_flags_classify(what, records, hits, n_ref):
    """spsp_extract_flags_classify_host: a word (matched, unmatched, best=<j>, listed=<j>) and classify's rows (records, hits[n, top])
    -> keep: np.uint8[n]"""
    records = np.ascontiguousarray(records, dtype=CLASSIFY_RECORD_DTYPE)
    hits = np.ascontiguousarray(hits, dtype=CLASSIFY_HIT_DTYPE)
    n = len(records)
    if hits.ndim != 2 or hits.shape[0] != n:
        raise ValueError("extract_flags_classify: hits[n_records, top]")
    keep = np.zeros(max(n, 1), dtype=np.uint8)
    _check(lib().spsp_extract_flags_classify_host(what.encode(), records.ctypes.data if n else None, hits.ctypes.data if n else None, n, hits.shape[1], n_ref,
                                                  keep.ctypes.data))
    return keep[:n]


def extract_flags_taxonomy(what, records, size):
    """spsp_extract_flags_taxonomy_host: a word (classified, unclassified, taxon=<t>, clade=<t>), the taxonomy's rows and the tree's
    subtree sizes (taxonomy_lineages()["size"]) -> keep: np.uint8[n]"""
    records = np.ascontiguousarray(records, dtype=TAXONOMY_RECORD_DTYPE)
    size = np.ascontiguousarray(size, dtype=np.uint32)
    n = len(records)
    keep = np.zeros(max(n, 1), dtype=np.uint8)
    _check(lib().spsp_extract_flags_taxonomy_host(what.encode(), records.ctypes.data if n else None, n, size.ctypes.data if len(size) else None, len(size),
                                                  keep.ctypes.data))
    return keep[:n]


SPLIT_DROP = 0xFFFFFFFF


def split_plan():
    """spsp_split_plan_host: what the split's kernels cut at -> dict(stretch_bytes: the bytes of the output one workgroup of the copy
    owns, record_tile: the records (and the sorted runs) per workgroup of the run table's and the offsets' passes, sort_tile: the
    pairs per workgroup of the radix sort, max_bins)"""
    a, b, c, d = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    _check(lib().spsp_split_plan_host(C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
    return {"stretch_bytes": a.value, "record_tile": b.value, "sort_tile": c.value, "max_bins": d.value}


def records_split(text, bins, n_bins, begin=None):
    """spsp_records_split_host: every record of `text` in the slice of its bin (SPLIT_DROP: nowhere), bin behind bin, record order
    inside a bin, a newline appended to a last record that lacks one -> (bytes, bin_off: np.uint64[n_bins + 1], bin_records:
    np.uint64[n_bins]).  begin: the records' starts (records_extents(text) when None)"""
    if begin is None:
        begin = records_extents(text)
    text = np.frombuffer(bytes(text), dtype=np.uint8)
    begin = np.ascontiguousarray(begin, dtype=np.uint64)
    bins = np.ascontiguousarray(bins, dtype=np.uint32)
    if len(begin) < 1 or len(bins) != len(begin) - 1:
        raise ValueError("records_split: one bin per record and n_rec + 1 starts")
    out, n_out, off, rec = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_void_p()
    _check(lib().spsp_records_split_host(text.ctypes.data if len(text) else None, len(text), begin.ctypes.data, len(bins), bins.ctypes.data if len(bins) else None,
                                         n_bins, C.byref(out), C.byref(n_out), C.byref(off), C.byref(rec)))
    return (_take(out, n_out.value), np.frombuffer(_take(off, (n_bins + 1) * 8), dtype=np.uint64).copy(),
            np.frombuffer(_take(rec, n_bins * 8), dtype=np.uint64).copy())


def split_bins_classify(what, records, hits, n_ref):
    """spsp_split_bins_classify_host: the word `best` and classify's rows (records, hits[n, top]) -> (bins: np.uint32[n], n_bins =
    n_ref + 1): the rank-1 match's list position, n_ref for a record without a match"""
    records = np.ascontiguousarray(records, dtype=CLASSIFY_RECORD_DTYPE)
    hits = np.ascontiguousarray(hits, dtype=CLASSIFY_HIT_DTYPE)
    n = len(records)
    if hits.ndim != 2 or hits.shape[0] != n:
        raise ValueError("split_bins_classify: hits[n_records, top]")
    bins, n_bins = np.zeros(max(n, 1), dtype=np.uint32), C.c_uint32()
    _check(lib().spsp_split_bins_classify_host(what.encode(), records.ctypes.data if n else None, hits.ctypes.data if n else None, n, hits.shape[1], n_ref,
                                               bins.ctypes.data, C.byref(n_bins)))
    return bins[:n], n_bins.value


def split_bins_taxonomy(what, records, parent, depth):
    """spsp_split_bins_taxonomy_host: a word (taxon, depth=<d>), the taxonomy's rows and the tree's parents and depths
    (taxonomy_lineages()) -> (bins: np.uint32[n], n_bins = n_nodes + 1); unclassified records go to bin n_nodes"""
    records = np.ascontiguousarray(records, dtype=TAXONOMY_RECORD_DTYPE)
    parent = np.ascontiguousarray(parent, dtype=np.uint32)
    depth = np.ascontiguousarray(depth, dtype=np.uint32)
    if len(parent) != len(depth):
        raise ValueError("split_bins_taxonomy: one parent and one depth per node")
    n = len(records)
    bins, n_bins = np.zeros(max(n, 1), dtype=np.uint32), C.c_uint32()
    _check(lib().spsp_split_bins_taxonomy_host(what.encode(), records.ctypes.data if n else None, n, parent.ctypes.data if len(parent) else None,
                                               depth.ctypes.data if len(depth) else None, len(parent), bins.ctypes.data, C.byref(n_bins)))
    return bins[:n], n_bins.value


def split_word_check(what, taxonomy):
    """spsp_split_word_check_host: only the refusals of a split word (taxonomy: the rows will be a taxonomy's)"""
    _check(lib().spsp_split_word_check_host(what.encode(), 1 if taxonomy else 0))


def split_csv(file_prefix, names, last_name, bin_records, bin_off, suffix, bin_off_mates=None, suffix_mates=None):
    """spsp_split_csv_host: the text of <prefix>_split.csv.gz -- one line per bin with records; names: n_bins - 1, last_name: the
    last bin's (unmatched, unclassified); with bin_off_mates the paired columns"""
    bin_records = np.ascontiguousarray(bin_records, dtype=np.uint64)
    bin_off = np.ascontiguousarray(bin_off, dtype=np.uint64)
    n_bins = len(bin_records)
    if len(bin_off) != n_bins + 1 or len(names) != n_bins - 1:
        raise ValueError("split_csv: n_bins - 1 names, n_bins counts, n_bins + 1 offsets")
    arr, _alive = _paths_array(names)
    mates = None if bin_off_mates is None else np.ascontiguousarray(bin_off_mates, dtype=np.uint64)
    text, n = C.c_void_p(), C.c_uint64()
    _check(lib().spsp_split_csv_host(file_prefix.encode(), arr, last_name.encode(), n_bins, bin_records.ctypes.data, bin_off.ctypes.data, suffix.encode(),
                                     None if mates is None else mates.ctypes.data, None if suffix_mates is None else suffix_mates.encode(), C.byref(text),
                                     C.byref(n)))
    return _take(text, n.value)


def windows_plan():
    """spsp_windows_plan_host: what the windows' kernels cut at -> dict(stretch_bases, stretch_bases_packed: the output bases one
    workgroup of the copy owns in the ASCII and in the packed form; record_tile: the records per workgroup of the counting pass)"""
    a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
    _check(lib().spsp_windows_plan_host(C.byref(a), C.byref(b), C.byref(c)))
    return {"stretch_bases": a.value, "stretch_bases_packed": b.value, "record_tile": c.value}


def records_windows(rec_off, k, window):
    """spsp_records_windows_host: the counting rule from the records' base offsets alone -> (first_win: np.uint32[n_rec + 1],
    win_off: np.uint64[n_windows + 1], the windows' base offsets in the expanded text)"""
    rec_off = np.ascontiguousarray(rec_off, dtype=np.uint64)
    if len(rec_off) < 1:
        raise ValueError("records_windows: n_rec + 1 offsets")
    n_rec = len(rec_off) - 1
    first = np.zeros(n_rec + 1, dtype=np.uint32)
    off, n_win, n_bases = C.c_void_p(), C.c_uint64(), C.c_uint64()
    _check(lib().spsp_records_windows_host(rec_off.ctypes.data, n_rec, k, window, first.ctypes.data, C.byref(off), C.byref(n_win), C.byref(n_bases)))
    return first, np.frombuffer(_take(off, (n_win.value + 1) * 8), dtype=np.uint64).copy()


def windows_expand(bases, rec_off, k, window):
    """spsp_windows_expand_host: the windows' bases back to back, as plain loops over ASCII bases -> (np.uint8 array, first_win,
    win_off): what the device pass is held against"""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    rec_off = np.ascontiguousarray(rec_off, dtype=np.uint64)
    if len(rec_off) < 1 or int(rec_off[-1]) > len(bases):
        raise ValueError("windows_expand: n_rec + 1 offsets that end inside the bases")
    n_rec = len(rec_off) - 1
    first = np.zeros(n_rec + 1, dtype=np.uint32)
    out, n_out, off, n_win = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
    _check(lib().spsp_windows_expand_host(bases.ctypes.data if len(bases) else None, rec_off.ctypes.data, n_rec, k, window, C.byref(out), C.byref(n_out),
                                          first.ctypes.data, C.byref(off), C.byref(n_win)))
    return (np.frombuffer(_take(out, n_out.value), dtype=np.uint8).copy(), first,
            np.frombuffer(_take(off, (n_win.value + 1) * 8), dtype=np.uint64).copy())


def windows_segments(call, keys, hit_keys, support, first_win, rec_off, k, window, n_bins):
    """spsp_windows_segments_host: the windows' calls (n_bins - 1: none) and addends -> (segments: SEGMENT_ROW_DTYPE[n_segments],
    mosaic: MOSAIC_ROW_DTYPE[n_rec]).  A call >= n_bins or a first_win that is not the rule's is refused, naming the record"""
    call, keys, hit_keys, support, first_win = (np.ascontiguousarray(x, dtype=np.uint32) for x in (call, keys, hit_keys, support, first_win))
    rec_off = np.ascontiguousarray(rec_off, dtype=np.uint64)
    n_rec = len(rec_off) - 1
    if n_rec < 0 or len(first_win) != n_rec + 1 or not (len(call) == len(keys) == len(hit_keys) == len(support)) or len(call) < int(first_win[-1]):
        raise ValueError("windows_segments: n_rec + 1 offsets and first windows, and one call and three addends per window")
    mosaic = np.zeros(max(n_rec, 1), dtype=MOSAIC_ROW_DTYPE)
    seg, n_seg = C.c_void_p(), C.c_uint64()
    ptr = lambda x: x.ctypes.data if len(x) else None
    _check(lib().spsp_windows_segments_host(ptr(call), ptr(keys), ptr(hit_keys), ptr(support), first_win.ctypes.data, rec_off.ctypes.data, n_rec, k, window, n_bins,
                                            C.byref(seg), C.byref(n_seg), mosaic.ctypes.data))
    return np.frombuffer(_take(seg, n_seg.value * SEGMENT_ROW_DTYPE.itemsize), dtype=SEGMENT_ROW_DTYPE).copy(), mosaic[:n_rec]


def segments_csv(segments, record_names, call_names, last_name):
    """spsp_segments_csv_host: the text of <prefix>_segments.csv.gz; call_names: n_bins - 1, last_name: the last bin's"""
    segments = np.ascontiguousarray(segments, dtype=SEGMENT_ROW_DTYPE)
    rn, _a = _paths_array(record_names)
    cn, _b = _paths_array(call_names)
    text, n = C.c_void_p(), C.c_uint64()
    _check(lib().spsp_segments_csv_host(segments.ctypes.data if len(segments) else None, len(segments), rn, len(record_names), cn, last_name.encode(),
                                        len(call_names) + 1, C.byref(text), C.byref(n)))
    return _take(text, n.value).decode()


def mosaic_csv(mosaic, record_names, call_names, last_name, precision=6):
    """spsp_mosaic_csv_host: the text of <prefix>_mosaic.csv.gz, one line per record"""
    mosaic = np.ascontiguousarray(mosaic, dtype=MOSAIC_ROW_DTYPE)
    if len(mosaic) != len(record_names):
        raise ValueError("mosaic_csv: one name per record")
    rn, _a = _paths_array(record_names)
    cn, _b = _paths_array(call_names)
    text, n = C.c_void_p(), C.c_uint64()
    _check(lib().spsp_mosaic_csv_host(mosaic.ctypes.data if len(mosaic) else None, len(mosaic), rn, cn, last_name.encode(), len(call_names) + 1, precision,
                                      C.byref(text), C.byref(n)))
    return _take(text, n.value).decode()


def _windows_result(first, n_rec, seg, n_seg, mos):
    return {"first_win": np.frombuffer(_take(first, (n_rec + 1) * 4), dtype=np.uint32).copy(),
            "segments": np.frombuffer(_take(seg, n_seg * SEGMENT_ROW_DTYPE.itemsize), dtype=SEGMENT_ROW_DTYPE).copy(),
            "mosaic": np.frombuffer(_take(mos, n_rec * MOSAIC_ROW_DTYPE.itemsize), dtype=MOSAIC_ROW_DTYPE).copy()}


def segments_plan():
    """spsp_segments_plan_host: what the segments' writer cuts at -> dict(line_bases, stretch_bytes)"""
    a, b = C.c_uint32(), C.c_uint32()
    _check(lib().spsp_segments_plan_host(C.byref(a), C.byref(b)))
    return {"line_bases": a.value, "stretch_bytes": b.value}


def windows_smooth(call, support, first_win, n_bins, q):
    """spsp_windows_smooth_host: a run of at most q windows between two runs of one call, each longer than q windows and in the same
    record, takes that call and support 0 -> (call, support, n_changed); the arguments stay as they are"""
    call = np.array(call, dtype=np.uint32)
    support = np.array(support, dtype=np.uint32)
    first_win = np.ascontiguousarray(first_win, dtype=np.uint32)
    if len(first_win) < 1 or len(call) != len(support):
        raise ValueError("windows_smooth: n_rec + 1 first windows, and one call and one support per window")
    if len(first_win) > 1 and int(first_win.max()) > len(call):
        raise ValueError("windows_smooth: first_win names windows that are not there")
    n = C.c_uint64()
    _check(lib().spsp_windows_smooth_host(call.ctypes.data if len(call) else None, support.ctypes.data if len(call) else None, first_win.ctypes.data, len(first_win) - 1,
                                          n_bins, q, C.byref(n)))
    return call, support, n.value


def segments_word_check(what, taxonomy=False, n_bins=0):
    """spsp_segments_word_check_host: only the refusals of a selection, a word or the command line's <word>:<min_bases>; n_bins: 0, or
    the bins <b> is held against"""
    _check(lib().spsp_segments_word_check_host(what.encode(), 1 if taxonomy else 0, n_bins))


def segments_select(segments, mosaic, n_bins, what, min_bases=1):
    """spsp_segments_select_host: -> (keep: np.uint8[n_segments], n_kept, n_bases)"""
    segments = np.ascontiguousarray(segments, dtype=SEGMENT_ROW_DTYPE)
    mosaic = np.ascontiguousarray(mosaic, dtype=MOSAIC_ROW_DTYPE)
    keep = np.zeros(max(len(segments), 1), dtype=np.uint8)
    n_kept, n_bases = C.c_uint64(), C.c_uint64()
    _check(lib().spsp_segments_select_host(segments.ctypes.data if len(segments) else None, len(segments), mosaic.ctypes.data if len(mosaic) else None, len(mosaic), n_bins,
                                           what.encode(), min_bases, keep.ctypes.data, C.byref(n_kept), C.byref(n_bases)))
    return keep[:len(segments)], n_kept.value, n_bases.value


def lift_plan():
    """spsp_lift_plan_host: what the lift's kernels cut at -> dict(tile_bytes, chunk_bytes)"""
    a, b = C.c_uint32(), C.c_uint32()
    _check(lib().spsp_lift_plan_host(C.byref(a), C.byref(b)))
    return {"tile_bytes": a.value, "chunk_bytes": b.value}


def _lift_base(base):
    base = np.ascontiguousarray(base, dtype=np.uint64)
    if base.ndim != 1:
        raise ValueError("lift: base is one global kept-base index per position")
    return base


def records_lift(text, base):
    """spsp_records_lift_host: the rule "raw coordinates" as plain loops.  text: a FASTA / FASTQ text (bytes); base: GLOBAL kept-base
    indices (rec_off[r] + p), non-decreasing -> (raw: np.uint64[n_q], record-relative positions among the record's sequence
    characters; rec: np.uint32[n_q]; raw_length: np.uint64[n_rec], every record's sequence characters)"""
    text = bytes(text)
    base = _lift_base(base)
    buf = (C.c_char * max(len(text), 1)).from_buffer_copy(text or b"\0")
    n_q = len(base)
    raw, rec = np.zeros(max(n_q, 1), dtype=np.uint64), np.zeros(max(n_q, 1), dtype=np.uint32)
    n_rec = C.c_uint32(0)
    _check(lib().spsp_records_lift_host(C.addressof(buf), len(text), None, 0, None, None, None, C.byref(n_rec)))   # the records first: raw_length's room
    raw_length = np.zeros(n_rec.value, dtype=np.uint64)
    _check(lib().spsp_records_lift_host(C.addressof(buf), len(text), base.ctypes.data if n_q else None, n_q, raw.ctypes.data, rec.ctypes.data, raw_length.ctypes.data,
                                        C.byref(n_rec)))
    return raw[:n_q], rec[:n_q], raw_length


def segments_bed(segments, raw_begin, raw_end, record_names, call_names, last_name):
    """spsp_segments_bed_host: the text of <prefix>_segments.bed -> bytes.  raw_begin, raw_end: one per segment"""
    segments = np.ascontiguousarray(segments, dtype=SEGMENT_ROW_DTYPE)
    raw_begin, raw_end = np.ascontiguousarray(raw_begin, dtype=np.uint64), np.ascontiguousarray(raw_end, dtype=np.uint64)
    if len(raw_begin) != len(segments) or len(raw_end) != len(segments):
        raise ValueError("segments_bed: one raw_begin and one raw_end per segment")
    rn, _a = _paths_array(record_names)
    cn, _b = _paths_array(call_names)
    text, n = C.c_void_p(), C.c_uint64()
    _check(lib().spsp_segments_bed_host(segments.ctypes.data if len(segments) else None, len(segments), raw_begin.ctypes.data if len(segments) else None,
                                        raw_end.ctypes.data if len(segments) else None, rn, len(record_names), cn, last_name.encode(), len(call_names) + 1, C.byref(text),
                                        C.byref(n)))
    return _take(text, n.value)


def segments_fasta(bases, rec_off, segments, record_names, call_names, last_name, keep=None):
    """spsp_segments_fasta_host: the text of <prefix>_segments.fa as plain loops over the ASCII bases of all records -> bytes.  keep:
    None (every segment) or a flag per segment; call_names: n_bins - 1, last_name: the last bin's"""
    bases = np.ascontiguousarray(np.frombuffer(bases, dtype=np.uint8) if isinstance(bases, (bytes, bytearray)) else bases, dtype=np.uint8)
    rec_off = np.ascontiguousarray(rec_off, dtype=np.uint64)
    segments = np.ascontiguousarray(segments, dtype=SEGMENT_ROW_DTYPE)
    if len(rec_off) < 1 or len(rec_off) - 1 != len(record_names):
        raise ValueError("segments_fasta: n_rec + 1 offsets and one name per record")
    if keep is not None:
        keep = np.ascontiguousarray(keep, dtype=np.uint8)
        if len(keep) != len(segments):
            raise ValueError("segments_fasta: one flag per segment")
    rn, _a = _paths_array(record_names)
    cn, _b = _paths_array(call_names)
    text, n = C.c_void_p(), C.c_uint64()
    _check(lib().spsp_segments_fasta_host(bases.ctypes.data if len(bases) else None, len(bases), rec_off.ctypes.data, len(rec_off) - 1,
                                          segments.ctypes.data if len(segments) else None, len(segments), keep.ctypes.data if keep is not None and len(keep) else None,
                                          rn, cn, last_name.encode(), len(call_names) + 1, C.byref(text), C.byref(n)))
    return _take(text, n.value)


def windows_word_check(what, taxonomy):
    """spsp_windows_word_check_host: only the refusals of a windows call word (taxonomy: the rows will be a taxonomy's)"""
    _check(lib().spsp_windows_word_check_host(what.encode(), 1 if taxonomy else 0))


def taxonomy_csv(records, record_names, parent, node_names, precision=6):
    """spsp_taxonomy_csv_host: records (TAXONOMY_RECORD_DTYPE), their names, the tree's parents and its nodes' names -> the text of
    <prefix>_taxonomy.csv.gz"""
    records = np.ascontiguousarray(records, dtype=TAXONOMY_RECORD_DTYPE)
    parent = np.ascontiguousarray(parent, dtype=np.uint32)
    if len(record_names) != len(records) or len(node_names) != len(parent):
        raise ValueError("taxonomy_csv: one name per record and per node")
    r_arr, _a = _paths_array(record_names)
    n_arr, _b = _paths_array(node_names)
    out, ln = C.c_void_p(), C.c_uint64()
    _check(lib().spsp_taxonomy_csv_host(records.ctypes.data if len(records) else None, len(records), r_arr, parent.ctypes.data if len(parent) else None,
                                        len(parent), n_arr, precision, C.byref(out), C.byref(ln)))
    return _take(out, ln.value)


def taxonomy_report_csv(records, parent, node_names, ref_node):
    """spsp_taxonomy_report_csv_host: the same rows and the references' nodes -> the text of <prefix>_taxonomy_report.csv.gz"""
    records = np.ascontiguousarray(records, dtype=TAXONOMY_RECORD_DTYPE)
    parent = np.ascontiguousarray(parent, dtype=np.uint32)
    ref_node = np.ascontiguousarray(ref_node, dtype=np.uint32)
    if len(node_names) != len(parent):
        raise ValueError("taxonomy_report_csv: one name per node")
    n_arr, _b = _paths_array(node_names)
    out, ln = C.c_void_p(), C.c_uint64()
    _check(lib().spsp_taxonomy_report_csv_host(records.ctypes.data if len(records) else None, len(records), parent.ctypes.data if len(parent) else None,
                                               len(parent), n_arr, ref_node.ctypes.data if len(ref_node) else None, len(ref_node), C.byref(out), C.byref(ln)))
    return _take(out, ln.value)


def groups_labels(text, n):
    """spsp_groups_labels_host: the text of a labels file (one label per line, in list order) for n sketches -> (group np.uint32[n],
    names: the G labels in the order of their first appearance)"""
    if isinstance(text, str):
        text = text.encode()
    group = np.zeros(max(n, 1), dtype=np.uint32)
    G, names, ln = C.c_uint32(), C.c_void_p(), C.c_uint64()
    _check(lib().spsp_groups_labels_host(text, len(text), n, group.ctypes.data, C.byref(G), C.byref(names), C.byref(ln)))
    blob = _take(names, ln.value)
    return group[:n], [x.decode() for x in blob.split(b"\0")[:G.value]]


def groups_bounds(group, n_groups, num, den, onum=0, oden=1):
    """spsp_groups_bounds_host: labels (0 .. n_groups-1 per sketch) and the two thresholds as fractions -> (size, in_min, out_max),
    np.uint32[n_groups] each: in_min = ceil(num * size / den), out_max = floor(onum * (n - size) / oden)"""
    group = np.ascontiguousarray(group, dtype=np.uint32)
    out = [np.zeros(max(n_groups, 1), dtype=np.uint32) for _ in range(3)]
    _check(lib().spsp_groups_bounds_host(group.ctypes.data if len(group) else None, len(group), n_groups, num, den, onum, oden, *[a.ctypes.data for a in out]))
    return tuple(a[:n_groups] for a in out)


def groups_csv(rows, names, precision=6):
    """spsp_groups_csv_host: group rows (GROUP_ROW_DTYPE array) and the groups' names -> the text of <prefix>_groups.csv.gz"""
    rows = np.ascontiguousarray(rows, dtype=GROUP_ROW_DTYPE)
    if len(names) != len(rows):
        raise ValueError("groups_csv: one name per group")
    arr, _alive = _paths_array(names)
    out, ln = C.c_void_p(), C.c_uint64()
    _check(lib().spsp_groups_csv_host(rows.ctypes.data if len(rows) else None, len(rows), arr, precision, C.byref(out), C.byref(ln)))
    return _take(out, ln.value)


def groups_members_csv(members, sketch_names, group, card, rows, names, precision=6):
    """spsp_groups_members_csv_host: member rows (GROUP_MEMBER_ROW_DTYPE array), the sketches' names, labels and key counts, the group
    rows and the groups' names -> the text of <prefix>_members.csv.gz"""
    members = np.ascontiguousarray(members, dtype=GROUP_MEMBER_ROW_DTYPE)
    rows = np.ascontiguousarray(rows, dtype=GROUP_ROW_DTYPE)
    group = np.ascontiguousarray(group, dtype=np.uint32)
    card = np.ascontiguousarray(card, dtype=np.uint64)
    n = len(members)
    if len(sketch_names) != n or len(group) != n or len(card) != n or len(names) != len(rows):
        raise ValueError("groups_members_csv: one name, label and key count per sketch, one name per group")
    s_arr, _a = _paths_array(sketch_names)
    g_arr, _b = _paths_array(names)
    out, ln = C.c_void_p(), C.c_uint64()
    _check(lib().spsp_groups_members_csv_host(members.ctypes.data if n else None, n, s_arr, group.ctypes.data if n else None, card.ctypes.data if n else None,
                                              rows.ctypes.data if len(rows) else None, len(rows), g_arr, precision, C.byref(out), C.byref(ln)))
    return _take(out, ln.value)


def sketches_from_payloads(payloads):
    """Parse sketch payloads IN FILE ORDER, as the comparator reads them: besides sketch_parse this applies the
    merge's first-read rule (spsp_sketch_chain_host), which gives an empty sketch one phantom key when k == m."""
    out = []
    buf = None
    for pl in payloads:
        sk = sketch_parse(pl)
        if buf is None:
            buf = C.create_string_buffer(b"A" * 16, 16)
        has, mn, lo, hi = C.c_int32(), C.c_uint32(), C.c_uint64(), C.c_uint64()
        _check(lib().spsp_sketch_chain_host(pl, len(pl), out[0].k if out else sk.k, out[0].m if out else sk.m, buf,
                                            C.byref(has), C.byref(mn), C.byref(lo), C.byref(hi)))
        if has.value and len(sk) == 0:
            sk = Sketch(sk.k, sk.m, np.array([mn.value], np.uint32), np.array([lo.value], np.uint64),
                        np.array([hi.value], np.uint64))
        out.append(sk)
    return out


def sort_csv(csv_text, fof_text):
    """sortCSV on gunzipped CSV bytes + file-of-files bytes -> reordered CSV bytes"""
    out, n = C.c_void_p(), C.c_uint64()
    _check(lib().spsp_sort_csv_host(csv_text, len(csv_text), fof_text, len(fof_text), C.byref(out), C.byref(n)))
    return _take(out, n.value)


def read_file(path):
    out, ln = C.c_void_p(), C.c_uint64()
    _check(lib().spsp_read_file_host(path.encode(), C.byref(out), C.byref(ln)))
    return _take(out, ln.value)


def write_gz(path, data, level=9):
    _check(lib().spsp_write_gz_host(path.encode(), data, len(data), level))


def sketch_files(fasta_paths, out_paths, k=31, m=11, s=1000.0, abundance=1, threads=8, device=0, flags=SPSP_SCAN_DEFAULT, devices=None):
    """many FASTA or FASTQ files -> many sketch files on `threads` workers, one context (HIP stream) each (spsp_sketch_files).
    Returns (per-file list of (rc, stats dict or None, error text or None), stage seconds summed over the workers)."""
    n = len(fasta_paths)
    p = make_params(k, m, s, abundance, flags)
    ins = (C.c_char_p * n)(*[x.encode() for x in fasta_paths])
    outs = (C.c_char_p * n)(*[x.encode() for x in out_paths])
    res = [None] * n
    started = []

    def on_file(user, i, phase, rc, st, err):
        if phase == 0:
            started.append(i)
        else:
            res[i] = (rc, {f: getattr(st.contents, f) for f, _ in SketchStats._fields_} if rc == 0 else None, err.decode() if err else None)
    cb = FILE_CALLBACK(on_file)
    times = StageTimes()
    if devices is not None:         # spsp_sketch_files_multi: the batches dealt over these devices
        devs = (C.c_int * len(devices))(*devices)
        rc = lib().spsp_sketch_files_multi(devs, len(devices), C.byref(p), float(s), ins, outs, n, threads, cb, None, C.byref(times))
    else:
        rc = lib().spsp_sketch_files(device, C.byref(p), float(s), ins, outs, n, threads, cb, None, C.byref(times))
    if rc != 0 and not any(r is not None and r[0] != 0 for r in res):
        _check(rc)
    return res, {f: getattr(times, f) for f, _ in StageTimes._fields_}, started


def sketch_files_release(device=-1):
    """release the contexts and pinned buffers spsp_sketch_files keeps between calls"""
    lib().spsp_sketch_files_release(device)


def device_count():
    """spsp_device_count: gfx950 devices visible to this process (initialises HIP)"""
    return int(lib().spsp_device_count())


def _paths_array(paths):
    """a `const char* const*` over `paths` for the C side, and what must stay alive while it is used.  Thousands of paths: ONE
    encode of the joined names and pointer arithmetic in numpy (10 000 c_char_p objects made one by one were 5 ms of a 37 ms
    spsp_compare_files call); anything that is not plain ASCII takes the plain road."""
    n = len(paths)
    if n >= 256:
        joined = "\0".join(paths)
        blob = joined.encode() + b"\0"
        if len(blob) == len(joined) + 1:                                          # ASCII: a character is a byte
            lens = np.fromiter(map(len, paths), dtype=np.uint64, count=n)
            if int(lens.sum()) + n == len(blob):                                  # (no name holds a NUL)
                buf = C.create_string_buffer(blob, len(blob))
                ptrs = np.empty(n, dtype=np.uint64)
                ptrs[0] = 0
                np.cumsum(lens[:-1] + np.uint64(1), out=ptrs[1:])
                ptrs += np.uint64(C.addressof(buf))
                return ptrs.ctypes.data_as(C.POINTER(C.c_char_p)), (buf, ptrs)
    arr = (C.c_char_p * n)(*[x.encode() for x in paths])
    return arr, (arr,)


def compare_files_multi(devices, paths, out_prefix, n_query=None, precision=6, min_threshold=0.0, rate=0.0):
    """spsp_compare_files_multi(_rate): the comparator split by key over one context per entry of `devices` -> stage seconds.
    rate: 0.0 = the headers' sampling rates are ignored; a rate or "auto" = every sketch is brought down to it on its device first"""
    n = len(paths)
    devs = (C.c_int * len(devices))(*devices)
    arr, _alive = _paths_array(paths)
    st = StageTimes()
    r = _rate_arg(rate)
    if r == RATE_AS_IS:
        _check(lib().spsp_compare_files_multi(devs, len(devices), arr, n, n if n_query is None else n_query, precision, float(min_threshold),
                                              out_prefix.encode(), 0, C.byref(st)))
    else:
        _check(lib().spsp_compare_files_multi_rate(devs, len(devices), arr, n, n if n_query is None else n_query, precision, float(min_threshold),
                                                   out_prefix.encode(), 0, C.byref(st), r))
    return {f: getattr(st, f) for f, _ in StageTimes._fields_}


def stream_create_cus(device, first_cu, n_cu):
    """a HIP stream (handle as int) whose kernels run on logical CUs [first_cu, first_cu + n_cu) only"""
    h = C.c_void_p()
    _check(lib().spsp_stream_create_cus(device, first_cu, n_cu, C.byref(h)))
    return h.value


def stream_destroy(device, stream):
    _check(lib().spsp_stream_destroy(device, C.c_void_p(stream)))


class Context:
    """One HIP device + one stream (spsp_create).  Raises SpspError without a gfx950 GPU."""

    def __init__(self, device=0, stream=None):
        self._h = C.c_void_p()
        _check(lib().spsp_create(device, C.c_void_p(stream) if stream else None, C.byref(self._h)))

    def close(self):
        if self._h:
            lib().spsp_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def to_host(self, d_ptr, count, dtype):
        """copy `count` items of numpy dtype from a device buffer returned by this context."""
        out = np.zeros(count, dtype=dtype)
        _check(lib().spsp_copy_to_host(self._h, out.ctypes.data, d_ptr, out.nbytes))
        return out

    # ---- measurement
    def timing_enable(self, on=True, kinds=TIME_ALL):
        """HIP-event brackets for the regions in `kinds` (TIME_DENSE | TIME_SCAN | TIME_ACCUMULATE | TIME_COMPARE)"""
        _check(lib().spsp_timing_enable(self._h, int(kinds) if on else 0))

    def timing_sample(self, every):
        """bracket only every `every`-th region (the event packets themselves delay a pipelined stream)"""
        _check(lib().spsp_timing_sample(self._h, every))

    def timing_read(self):
        """HIP-event totals since the last read (synchronises the stream) as a dict."""
        t = Timing()
        _check(lib().spsp_timing_read(self._h, C.byref(t)))
        return {f: getattr(t, f) for f, _ in Timing._fields_}

    def measure_hbm(self, nbytes=1 << 30, reps=10):
        """streaming copy / read rates of this device on this context's stream (roofline denominator) as a dict"""
        r = HbmRates()
        _check(lib().spsp_measure_hbm_device(self._h, nbytes, reps, C.byref(r)))
        return {f: getattr(r, f) for f, _ in HbmRates._fields_}

    # ---- path A
    def scan(self, params, bases, rec_off):
        """cleaned ASCII records -> structured array of selected super-k-mers (genome order)."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        rec_off = np.ascontiguousarray(rec_off, dtype=np.uint64)
        out, n = C.c_void_p(), C.c_uint64()
        _check(lib().spsp_scan(self._h, C.byref(params), bases.ctypes.data, rec_off.ctypes.data, len(rec_off) - 1,
                               C.byref(out), C.byref(n)))
        if n.value == 0:
            return np.zeros(0, dtype=SUPERKMER_DTYPE)
        return np.frombuffer(_take(out, n.value * SUPERKMER_DTYPE.itemsize), dtype=SUPERKMER_DTYPE).copy()

    def scan_device(self, params, d_bases, n_bases, d_rec_off, n_rec):
        """device pointers in, device pointer out: returns (d_out, n_out); d_out is owned by the
        context and valid until its next scan call."""
        out, n = C.c_void_p(), C.c_uint64()
        _check(lib().spsp_scan_device(self._h, C.byref(params), d_bases, n_bases, d_rec_off, n_rec, C.byref(out),
                                      C.byref(n)))
        return out.value, n.value

    def pack_bases_device(self, d_bases, n_bases):
        """cleaned ASCII bases on the device -> 2-bit packed buffer owned by the context (for SPSP_SCAN_PACKED_INPUT)"""
        out = C.c_void_p()
        _check(lib().spsp_pack_bases_device(self._h, d_bases, n_bases, C.byref(out)))
        return out.value

    def scan_device_begin(self, params, d_bases, n_bases, d_rec_off, n_rec):
        """queue the scan on the context's stream and return; collect with scan_device_end()"""
        _check(lib().spsp_scan_device_begin(self._h, C.byref(params), d_bases, n_bases, d_rec_off, n_rec))

    def scan_device_end(self):
        out, n = C.c_void_p(), C.c_uint64()
        _check(lib().spsp_scan_device_end(self._h, C.byref(out), C.byref(n)))
        return out.value, n.value

    def set_cu_count(self, n_cu, dense_blocks_per_cu=1):
        """how many CUs the context's stream owns (0 = the whole device) and how many dense workgroups go on each
        (2 for a stream that has its CUs to itself): sizes the dense pass's grid"""
        _check(lib().spsp_set_cu_count(self._h, n_cu, dense_blocks_per_cu))

    def scan_tail_stream(self, on=True, stream=None):
        """sparse stages of the scan on a second stream (None = one the context creates)"""
        _check(lib().spsp_scan_tail_stream(self._h, 1 if on else 0, stream))

    def wait_dense(self, scanner):
        """work queued on this context from now on starts behind `scanner`'s latest dense pass"""
        _check(lib().spsp_wait_dense(self._h, scanner._h))

    def wait_stream(self, other):
        """work queued on this context from now on starts behind everything queued on `other` so far"""
        _check(lib().spsp_wait_stream(self._h, other._h))

    def scan_hits_device(self, params, d_bases, n_bases):
        n = C.c_uint64()
        _check(lib().spsp_scan_hits_device(self._h, C.byref(params), d_bases, n_bases, C.byref(n)))
        return n.value

    def count_superkmers_device(self, params, d_bases, n_bases, d_rec_off, n_rec):
        """total_superkmer_number of print_stat: every super-k-mer of the input, selected or not"""
        n = C.c_uint64()
        _check(lib().spsp_count_superkmers_device(self._h, C.byref(params), d_bases, n_bases, d_rec_off, n_rec, C.byref(n)))
        return n.value

    def stats_counts(self):
        """spsp_stats_counts: which form answered -> dict(scan_form, scan_left: the last collected scan (0 none or empty, 1 by segments,
        2 the product scan, 3 the product scan after the segment count left a chain unfinished) and the chains it reported;
        count_form, count_chains: the last super-k-mer count (1 by segments, 2 the chunk kernels, 3 the chunk kernels after a
        hand-over) and the chains that left their tile's halo)"""
        counts = (C.c_uint32 * 4)()
        _check(lib().spsp_stats_counts(self._h, counts))
        return dict(zip(("scan_form", "scan_left", "count_form", "count_chains"), (int(c) for c in counts)))

    def clean_fasta_device(self, d_text, n_text):
        """raw FASTA text in HBM -> (d_bases, n_bases, d_rec_off, n_rec), context-owned device buffers."""
        b, o, nb, nr = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint32()
        _check(lib().spsp_fasta_clean_device(self._h, d_text, n_text, C.byref(b), C.byref(nb), C.byref(o), C.byref(nr)))
        return b.value, nb.value, o.value, nr.value

    def clean_fasta_packed_device(self, d_text, n_text):
        """raw FASTA text in HBM -> (d_packed 2-bit words, n_bases, d_rec_off, n_rec), context-owned device buffers"""
        b, o, nb, nr = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint32()
        _check(lib().spsp_fasta_clean_packed_device(self._h, d_text, n_text, C.byref(b), C.byref(nb), C.byref(o), C.byref(nr)))
        return b.value, nb.value, o.value, nr.value

    def clean_fastq_device(self, d_text, n_text):
        """raw FASTQ text in HBM -> (d_bases, n_bases, d_rec_off, n_rec), one record per read, context-owned device buffers;
        a malformed record raises SpspError naming its 0-based index"""
        b, o, nb, nr = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint32()
        _check(lib().spsp_fastq_clean_device(self._h, d_text, n_text, C.byref(b), C.byref(nb), C.byref(o), C.byref(nr)))
        return b.value, nb.value, o.value, nr.value

    def clean_fastq_packed_device(self, d_text, n_text):
        """raw FASTQ text in HBM -> (d_packed 2-bit words, n_bases, d_rec_off, n_rec), context-owned device buffers"""
        b, o, nb, nr = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint32()
        _check(lib().spsp_fastq_clean_packed_device(self._h, d_text, n_text, C.byref(b), C.byref(nb), C.byref(o), C.byref(nr)))
        return b.value, nb.value, o.value, nr.value

    def clean_batch(self, slab, files, packed=False):
        """the batch form of the ingest: slab = host bytes laid out as the file pipeline lays a batch out, files = (offset,
        text length, BATCH_* flags) per file -> (d_bases or d_packed, n_bases, d_rec_off, n_rec, rec_base np.uint32 per
        tile, bad np.uint64 per file: ~0 or (first malformed record in the batch) << 8 | rule)"""
        arr = (BatchFile * max(1, len(files)))(*[BatchFile(o, n, fl, 0) for o, n, fl in files])
        rec_base = np.zeros(len(slab) // 4096 + 1, dtype=np.uint32)
        bad = np.zeros(max(1, len(files)), dtype=np.uint64)
        b, o, nb, nr = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint32()
        _check(lib().spsp_ingest_batch(self._h, bytes(slab), len(slab), arr, len(files), 1 if packed else 0, C.byref(b), C.byref(nb),
                                       C.byref(o), C.byref(nr), rec_base.ctypes.data, bad.ctypes.data))
        return b.value, nb.value, o.value, nr.value, rec_base[:len(slab) // 4096], bad[:len(files)]

    def sketch_text(self, text, k=31, m=11, s=1000.0, abundance=1, flags=SPSP_SCAN_DEFAULT):
        """FASTA or FASTQ bytes (FASTQ: the first byte is '@') -> (payload, stats) with ingest, scan and gather on the GPU."""
        p = make_params(k, m, s, abundance, flags)
        out, n, st = C.c_void_p(), C.c_uint64(), SketchStats()
        _check(lib().spsp_sketch_text(self._h, C.byref(p), float(s), text, len(text), C.byref(out), C.byref(n), C.byref(st)))
        return _take(out, n.value), {f: getattr(st, f) for f, _ in SketchStats._fields_}

    def sketch_build_device(self, params, rate, bases, rec_off, superkmers, file_sk, packed=False):
        """super-k-mer stream of len(file_sk) - 1 files (file f: superkmers[file_sk[f]:file_sk[f + 1]], `rec` counting over all
        records) -> ([payload per file], [counter dict per file]) by the builder on the device (spsp_sketch_build_device)."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        rec_off = np.ascontiguousarray(rec_off, dtype=np.uint64)
        sk = np.ascontiguousarray(superkmers, dtype=SUPERKMER_DTYPE)
        fsk = np.ascontiguousarray(file_sk, dtype=np.uint32)
        n_files = len(fsk) - 1
        out = C.c_void_p()
        off = np.zeros(n_files + 1, dtype=np.uint64)
        cnt = np.zeros(4 * n_files, dtype=np.uint64)
        _check(lib().spsp_sketch_build_device(self._h, C.byref(params), float(rate), bases.ctypes.data, rec_off.ctypes.data, len(rec_off) - 1,
                                              sk.ctypes.data, len(sk), fsk.ctypes.data, n_files, 1 if packed else 0, C.byref(out),
                                              off.ctypes.data, cnt.ctypes.data))
        data = _take(out, int(off[-1]))
        names = ("actual_minimizer_number", "seen_kmers_at_reconstruction", "seen_superkmers_at_reconstruction",
                 "seen_max_superkmers_at_reconstruction")
        return ([data[int(off[f]):int(off[f + 1])] for f in range(n_files)],
                [dict(zip(names, (int(x) for x in cnt[4 * f: 4 * f + 4]))) for f in range(n_files)])

    def sketch_fasta(self, text, k=31, m=11, s=1000.0, abundance=1, flags=SPSP_SCAN_DEFAULT):
        """FASTA bytes -> (payload, stats): clean -> GPU scan -> sketch builder."""
        p = make_params(k, m, s, abundance, flags)
        bases, off = clean_fasta(text)
        sk = self.scan(p, bases, off)
        return sketch_build(p, s, bases, off, sk)

    def sketch_file(self, fasta_path, out_path, k=31, m=11, s=1000.0, abundance=1):
        p = make_params(k, m, s, abundance)
        st = SketchStats()
        _check(lib().spsp_sketch_file(self._h, C.byref(p), float(s), fasta_path.encode(), out_path.encode(),
                                      C.byref(st)))
        return {f: getattr(st, f) for f, _ in SketchStats._fields_}

    def sketch_decode_device(self, payloads):
        """list of gunzipped sketch payloads -> (k, m, d_minimizer, d_kmer_lo, d_kmer_hi or None, sk_off np.uint64[n+1]);
        the device pointers belong to the context (valid until its next decode / compare call)"""
        n = len(payloads)
        arr = (C.c_char_p * n)(*payloads)
        lens = (C.c_uint64 * n)(*[len(p) for p in payloads])
        k, m = C.c_uint32(), C.c_uint32()
        d_mn, d_lo, d_hi = C.c_void_p(), C.c_void_p(), C.c_void_p()
        sk_off = np.zeros(n + 1, dtype=np.uint64)
        _check(lib().spsp_sketch_decode_device(self._h, arr, lens, n, C.byref(k), C.byref(m), C.byref(d_mn), C.byref(d_lo),
                                                C.byref(d_hi), sk_off.ctypes.data_as(C.POINTER(C.c_uint64))))
        return k.value, m.value, d_mn.value, d_lo.value, d_hi.value, sk_off

    def scan_output_wait(self, reader):
        """this context's next scan writes its output only behind `reader`'s latest sketch_keys_device_begin"""
        _check(lib().spsp_scan_output_wait(self._h, reader._h))

    def compare_forget(self):
        """forget what earlier comparisons taught this context about its inputs (scheduling only: spsp_compare_forget)"""
        _check(lib().spsp_compare_forget(self._h))

    def compare_keys_unordered(self, on=True):
        """device-form comparisons of this context accept sketches whose keys are distinct but unsorted"""
        _check(lib().spsp_compare_keys_unordered(self._h, 1 if on else 0))

    def sketch_keys_device_begin(self, params, d_bases, n_bases, d_rec_off, d_sk, n_sk, first_rec, unordered=False):
        """queue: scan output -> comparator keys of the genomes whose record ranges `first_rec` (n_genomes + 1) gives"""
        fr = np.ascontiguousarray(first_rec, dtype=np.uint32)
        _check(lib().spsp_sketch_keys_device_begin(self._h, C.byref(params), d_bases, n_bases, d_rec_off, d_sk, n_sk, fr.ctypes.data, len(fr) - 1,
                                                   KEYS_UNORDERED if unordered else 0))
        self._keys_n = len(fr) - 1

    def sketch_keys_device_end(self):
        """-> (d_minimizer, d_kmer_lo, d_kmer_hi or None, sk_off np.uint64[n_genomes + 1]); device pointers belong to the context"""
        d_mn, d_lo, d_hi = C.c_void_p(), C.c_void_p(), C.c_void_p()
        sk_off = np.zeros(self._keys_n + 1, dtype=np.uint64)
        _check(lib().spsp_sketch_keys_device_end(self._h, C.byref(d_mn), C.byref(d_lo), C.byref(d_hi), sk_off.ctypes.data))
        return d_mn.value, d_lo.value, d_hi.value, sk_off

    def sketch_keys_big_genomes(self):
        """genomes of the last collected key extraction that were beyond the per-genome LDS forms (table in HBM instead)"""
        return int(lib().spsp_sketch_keys_big_genomes(self._h))

    def sketch_keys_device(self, params, d_bases, n_bases, d_rec_off, d_sk, n_sk, first_rec, unordered=False):
        self.sketch_keys_device_begin(params, d_bases, n_bases, d_rec_off, d_sk, n_sk, first_rec, unordered)
        return self.sketch_keys_device_end()

    def stage_times(self, reset=True):
        """wall seconds the whole-file drivers (sketch_file / compare_files) spent per stage on this context"""
        st = StageTimes()
        _check(lib().spsp_stage_times_read(self._h, C.byref(st), 1 if reset else 0))
        return {f: getattr(st, f) for f, _ in StageTimes._fields_}

    # ---- path B
    def compare(self, sketches, n_query=None):
        """list of Sketch -> (inter uint32[n,n] upper triangle, card uint64[n])."""
        n = len(sketches)
        nq = n if n_query is None else n_query
        views = (SketchView * max(n, 1))()
        use_hi = any(s.k > 32 for s in sketches)
        for i, s in enumerate(sketches):
            views[i].minimizer = s.minimizer.ctypes.data
            views[i].kmer_lo = s.kmer_lo.ctypes.data
            views[i].kmer_hi = s.kmer_hi.ctypes.data if use_hi else None
            views[i].n = len(s)
        inter = np.zeros((n, n), dtype=np.uint32)
        card = np.zeros(n, dtype=np.uint64)
        _check(lib().spsp_compare(self._h, views, n, nq, inter.ctypes.data, card.ctypes.data))
        return inter, card

    def compare_device(self, k, d_min, d_lo, d_hi, sk_off, n, row_first, row_stride, d_inter, n_query=None):
        sk_off = np.ascontiguousarray(sk_off, dtype=np.uint64)
        _check(lib().spsp_compare_device(self._h, k, d_min, d_lo, d_hi, sk_off.ctypes.data, n,
                                         n if n_query is None else n_query, row_first, row_stride, d_inter))

    def compare_device_begin(self, k, d_min, d_lo, d_hi, sk_off, n, row_first, row_stride, d_inter, n_query=None):
        sk_off = np.ascontiguousarray(sk_off, dtype=np.uint64)
        _check(lib().spsp_compare_device_begin(self._h, k, d_min, d_lo, d_hi, sk_off.ctypes.data, n,
                                               n if n_query is None else n_query, row_first, row_stride, d_inter))

    def compare_slots_device_begin(self, k, d_slots, parts, n, slot_cap, d_inter):
        _check(lib().spsp_compare_slots_device_begin(self._h, k, d_slots, parts, n, slot_cap, d_inter))

    def compare_end(self):
        _check(lib().spsp_compare_end(self._h))

    def partition_keys_device(self, k, d_min, d_lo, d_hi, sk_off, n, parts, slot_cap, d_slots):
        """Scatter this rank's sketch keys into `parts` exchange slots (include/spsp.h); asynchronous."""
        sk_off = np.ascontiguousarray(sk_off, dtype=np.uint64)
        _check(lib().spsp_partition_keys_device(self._h, k, d_min, d_lo, d_hi, sk_off.ctypes.data, n, parts, slot_cap,
                                                d_slots))

    def compare_slots_device(self, k, d_slots, parts, n, slot_cap, d_inter):
        """Partial pair matrix of the hash class this rank received (one slot per source rank)."""
        _check(lib().spsp_compare_slots_device(self._h, k, d_slots, parts, n, slot_cap, d_inter))

    def matrix_cells_device(self, d_inter, n, d_cells, cap, row_first=0, row_limit=None):
        """non-zero cells (i < j) of a dense pair matrix on the device as packed words i << 48 | j << 32 | count -> how many"""
        cnt = C.c_uint64()
        _check(lib().spsp_matrix_cells_device(self._h, d_inter, n, row_first, n if row_limit is None else row_limit, d_cells, cap, C.byref(cnt)))
        return cnt.value

    def compare_cells_device(self, k, d_min, d_lo, d_hi, sk_off, n, d_scratch, d_cells, cap, n_query=None):
        """all-vs-all with the pair matrix returned as packed non-zero cells (i << 48 | j << 32 | count) -> how many"""
        sk_off = np.ascontiguousarray(sk_off, dtype=np.uint64)
        cnt = C.c_uint64()
        try:
            _check(lib().spsp_compare_cells_device(self._h, k, d_min, d_lo, d_hi, sk_off.ctypes.data, n, n if n_query is None else n_query, d_scratch,
                                                   d_cells, cap, C.byref(cnt)))
        except SpspError as e:
            e.cells_needed = cnt.value
            raise
        return cnt.value

    def compare_slots_cells_device(self, k, d_slots, parts, n, slot_cap, d_scratch, d_cells, cap):
        """this rank's partial matrix of the key-partitioned split as packed non-zero cells -> how many"""
        cnt = C.c_uint64()
        try:
            _check(lib().spsp_compare_slots_cells_device(self._h, k, d_slots, parts, n, slot_cap, d_scratch, d_cells, cap, C.byref(cnt)))
        except SpspError as e:
            e.cells_needed = cnt.value          # ERR_OVERFLOW from too little room: how much there must be (spsp.h)
            raise
        return cnt.value

    def matrix_add_cells_device(self, d_inter, n, d_cells, n_cells):
        _check(lib().spsp_matrix_add_cells_device(self._h, d_inter, n, d_cells, n_cells))

    def compare_files(self, paths, out_prefix, n_query=None, precision=6, min_threshold=0.0, rate=0.0):
        """rate: 0.0 = the headers' sampling rates are ignored (the reference's behaviour); a rate, or "auto" for the coarsest
        of the files', = every sketch is brought down to it on the device before the comparison"""
        n = len(paths)
        nq = n if n_query is None else n_query
        arr, _alive = _paths_array(paths)
        r = _rate_arg(rate)
        if r == RATE_AS_IS:
            _check(lib().spsp_compare_files(self._h, arr, n, nq, precision, float(min_threshold), out_prefix.encode()))
        else:
            _check(lib().spsp_compare_files_rate(self._h, arr, n, nq, precision, float(min_threshold), out_prefix.encode(), 0, r))

    def keys_downsample_device(self, k, threshold_value, d_min, d_lo, d_hi, sk_off):
        """concatenated key arrays on the device -> (d_minimizer, d_kmer_lo, d_kmer_hi or None, sk_off np.uint64[n + 1]): the keys
        whose minimizer passes `threshold_value` (threshold(k, m, rate)), order kept, in arrays the context owns"""
        sk_off = np.ascontiguousarray(sk_off, dtype=np.uint64)
        n = len(sk_off) - 1
        o_mn, o_lo, o_hi = C.c_void_p(), C.c_void_p(), C.c_void_p()
        out = np.zeros(n + 1, dtype=np.uint64)
        _check(lib().spsp_keys_downsample_device(self._h, k, threshold_value, d_min, d_lo, d_hi, sk_off.ctypes.data, n,
                                                 C.byref(o_mn), C.byref(o_lo), C.byref(o_hi), out.ctypes.data))
        return o_mn.value, o_lo.value, o_hi.value, out

    def gather_device(self, k, d_min, d_lo, d_hi, sk_off, n, n_query, min_keys, max_rounds=0):
        """spsp_gather_device: greedy gather of the first n_query sketches against the others over concatenated sorted key
        arrays on the device -> rows (GATHER_ROW_DTYPE array ordered by (query, rank)); the room grows here on overflow"""
        sk_off = np.ascontiguousarray(sk_off, dtype=np.uint64)
        cap = 64
        for _ in range(2):
            rows = np.zeros(cap, dtype=GATHER_ROW_DTYPE)
            cnt = C.c_uint64()
            rc = lib().spsp_gather_device(self._h, k, d_min, d_lo, d_hi, sk_off.ctypes.data, n, n_query, min_keys, max_rounds,
                                          rows.ctypes.data, cap, C.byref(cnt))
            if rc != ERR_OVERFLOW or cnt.value <= cap:
                break
            cap = cnt.value
        _check(rc)
        return rows[:cnt.value].copy()

    def gather_files(self, paths, out_prefix, n_query, min_keys, max_rounds=0, precision=6, rate=0.0):
        """spsp_gather_files: sketch files (the n_query queries first) -> <out_prefix>_gather.csv.gz and the rows.
        rate: as compare_files (0.0, a rate, or "auto")"""
        n = len(paths)
        arr, _alive = _paths_array(paths)
        out, cnt = C.c_void_p(), C.c_uint64()
        _check(lib().spsp_gather_files(self._h, arr, n, n_query, precision, min_keys, max_rounds, out_prefix.encode(), 0, _rate_arg(rate),
                                       C.byref(out), C.byref(cnt)))
        return np.frombuffer(_take(out, cnt.value * GATHER_ROW_DTYPE.itemsize), dtype=GATHER_ROW_DTYPE).copy()

    def cluster_cells_device(self, d_cells, n_cells, card, n, metric, num, den):
        """spsp_cluster_cells_device: single-linkage clusters of sketches 0 .. n-1 from the packed cells (i << 48 | j << 32 | count)
        of their pair matrix on the device and the n key counts -> (rows: CLUSTER_ROW_DTYPE array of n, n_clusters, n_edges);
        linked iff count * den >= num * (c_i + c_j - count) (metric 0) or >= num * min(c_i, c_j) (metric 1)"""
        card = np.ascontiguousarray(card, dtype=np.uint64)
        if len(card) != n:
            raise ValueError("cluster_cells_device: one key count per sketch")
        rows = np.zeros(n, dtype=CLUSTER_ROW_DTYPE)
        nc, ne = C.c_uint64(), C.c_uint64()
        _check(lib().spsp_cluster_cells_device(self._h, d_cells, n_cells, card.ctypes.data, n, metric, num, den, rows.ctypes.data, C.byref(nc), C.byref(ne)))
        return rows, nc.value, ne.value

    def cluster_files(self, paths, out_prefix, metric, num, den, precision=6, rate=0.0):
        """spsp_cluster_files: sketch files -> <out_prefix>_clusters.csv.gz and (rows, n_clusters).  rate: as compare_files"""
        n = len(paths)
        arr, _alive = _paths_array(paths)
        out, nc = C.c_void_p(), C.c_uint64()
        _check(lib().spsp_cluster_files(self._h, arr, n, precision, metric, num, den, out_prefix.encode(), 0, _rate_arg(rate), C.byref(out), C.byref(nc)))
        return np.frombuffer(_take(out, n * CLUSTER_ROW_DTYPE.itemsize), dtype=CLUSTER_ROW_DTYPE).copy(), nc.value

    def representatives_cells_device(self, d_cells, n_cells, card, n, metric, num, den, weight=None):
        """spsp_representatives_cells_device: greedy representatives of sketches 0 .. n-1 from the packed cells (i << 48 | j << 32 |
        count) of their pair matrix on the device, the n key counts and, optionally, n weights (each below 2^47; None: the key
        counts) -> (rows: CLUSTER_ROW_DTYPE array of n, n_clusters, n_edges, rounds).  The link test is cluster_cells_device's"""
        card = np.ascontiguousarray(card, dtype=np.uint64)
        if len(card) != n:
            raise ValueError("representatives_cells_device: one key count per sketch")
        if weight is not None:
            weight = np.ascontiguousarray(weight, dtype=np.uint64)
            if len(weight) != n:
                raise ValueError("representatives_cells_device: one weight per sketch")
        rows = np.zeros(n, dtype=CLUSTER_ROW_DTYPE)
        nc, ne, nr = C.c_uint64(), C.c_uint64(), C.c_uint32()
        _check(lib().spsp_representatives_cells_device(self._h, d_cells, n_cells, card.ctypes.data, weight.ctypes.data if weight is not None else None,
                                                       n, metric, num, den, rows.ctypes.data, C.byref(nc), C.byref(ne), C.byref(nr)))
        return rows, nc.value, ne.value, nr.value

    def representatives_files(self, paths, out_prefix, metric, num, den, weight=None, precision=6, rate=0.0):
        """spsp_representatives_files: sketch files -> <out_prefix>_representatives.csv.gz and (rows, n_clusters).  weight: one per
        file, or None for the key counts.  rate: as compare_files"""
        n = len(paths)
        arr, _alive = _paths_array(paths)
        if weight is not None:
            weight = np.ascontiguousarray(weight, dtype=np.uint64)
            if len(weight) != n:
                raise ValueError("representatives_files: one weight per file")
        out, nc = C.c_void_p(), C.c_uint64()
        _check(lib().spsp_representatives_files(self._h, arr, n, precision, metric, num, den, weight.ctypes.data if weight is not None else None,
                                                out_prefix.encode(), 0, _rate_arg(rate), C.byref(out), C.byref(nc)))
        return np.frombuffer(_take(out, n * CLUSTER_ROW_DTYPE.itemsize), dtype=CLUSTER_ROW_DTYPE).copy(), nc.value

    def tree_cells_device(self, d_cells, n_cells, card, n, metric, num, den):
        """spsp_tree_cells_device: the single-linkage tree of sketches 0 .. n-1 from the packed cells (i << 48 | j << 32 | count) of
        their pair matrix on the device and the n key counts, over the cells that pass cluster_cells_device's link test at the
        floor num / den (num == 0: every cell that shares a key) -> (rows: TREE_ROW_DTYPE array, best merge first, n_edges: the
        candidate edges, rounds: the rounds that merged anything)"""
        card = np.ascontiguousarray(card, dtype=np.uint64)
        if len(card) != n:
            raise ValueError("tree_cells_device: one key count per sketch")
        rows = np.zeros(max(n, 1) - 1, dtype=TREE_ROW_DTYPE)
        nr, ne, rounds = C.c_uint64(), C.c_uint64(), C.c_uint32()
        _check(lib().spsp_tree_cells_device(self._h, d_cells, n_cells, card.ctypes.data, n, metric, num, den, rows.ctypes.data if len(rows) else None,
                                            C.byref(nr), C.byref(ne), C.byref(rounds)))
        return rows[:nr.value].copy(), ne.value, rounds.value

    def tree_files(self, paths, out_prefix, metric, num, den, precision=6, rate=0.0):
        """spsp_tree_files: sketch files -> <out_prefix>_tree.csv.gz, <out_prefix>_tree.nwk and the rows.  rate: as compare_files"""
        n = len(paths)
        arr, _alive = _paths_array(paths)
        out, nr = C.c_void_p(), C.c_uint64()
        _check(lib().spsp_tree_files(self._h, arr, n, precision, metric, num, den, out_prefix.encode(), 0, _rate_arg(rate), C.byref(out), C.byref(nr)))
        return np.frombuffer(_take(out, nr.value * TREE_ROW_DTYPE.itemsize), dtype=TREE_ROW_DTYPE).copy()

    def neighbours_cells_device(self, d_cells, n_cells, card, n, metric, num, den, top, n_query=None):
        """spsp_neighbours_cells_device: per row sketch (every sketch, or the first n_query) the best `top` partners at or above
        num / den from the packed cells (i << 48 | j << 32 | count) of the pair matrix on the device and the n key counts ->
        (rows: NEIGHBOUR_ROW_DTYPE array ordered by (sketch, rank), passing: np.uint32 per row sketch, n_pairs); the room grows
        here on overflow"""
        card = np.ascontiguousarray(card, dtype=np.uint64)
        if len(card) != n:
            raise ValueError("neighbours_cells_device: one key count per sketch")
        nq = n if n_query is None else n_query
        passing = np.zeros(max(min(n, nq), 1), dtype=np.uint32)
        cap = max(1, min(min(n, nq) * top, 2 * n_cells, 1 << 21))         # (every row there can be, up to 48 MB of them)
        for _ in range(2):
            rows = np.zeros(cap, dtype=NEIGHBOUR_ROW_DTYPE)
            cnt, pairs = C.c_uint64(), C.c_uint64()
            rc = lib().spsp_neighbours_cells_device(self._h, d_cells, n_cells, card.ctypes.data, n, nq, metric, num, den, top,
                                                    rows.ctypes.data, cap, C.byref(cnt), passing.ctypes.data, C.byref(pairs))
            if rc != ERR_OVERFLOW or cnt.value <= cap:
                break
            cap = cnt.value
        _check(rc)
        return rows[:cnt.value].copy(), passing[:min(n, nq)], pairs.value

    def neighbours_files(self, paths, out_prefix, top, metric=0, num=0, den=1, n_query=None, precision=6, rate=0.0):
        """spsp_neighbours_files: sketch files (the n_query queries first, or all versus all) -> <out_prefix>_neighbours.csv.gz
        and the rows.  rate: as compare_files (0.0, a rate, or "auto")"""
        n = len(paths)
        arr, _alive = _paths_array(paths)
        out, cnt = C.c_void_p(), C.c_uint64()
        _check(lib().spsp_neighbours_files(self._h, arr, n, n if n_query is None else n_query, precision, metric, num, den, top,
                                           out_prefix.encode(), 0, _rate_arg(rate), C.byref(out), C.byref(cnt)))
        return np.frombuffer(_take(out, cnt.value * NEIGHBOUR_ROW_DTYPE.itemsize), dtype=NEIGHBOUR_ROW_DTYPE).copy()

    def prevalence_device(self, k, d_min, d_lo, d_hi, sk_off, n, num, den, n_query=0, want_holders=False):
        """spsp_prevalence_device: how many references hold each key, over concatenated sorted key arrays on the device ->
        (rows: PREVALENCE_ROW_DTYPE array, one per row sketch -- every sketch, or the first n_query --, spectrum: np.uint64[R + 1]
        [, d_holders: the device address of the context's uint32 array of h per key occurrence, valid until the next call])"""
        sk_off = np.ascontiguousarray(sk_off, dtype=np.uint64)
        if len(sk_off) != n + 1:
            raise ValueError("prevalence_device: n + 1 sketch offsets")
        rows = np.zeros(max(n_query if n_query else n, 1), dtype=PREVALENCE_ROW_DTYPE)
        spectrum = np.zeros(max(n - n_query, 0) + 1, dtype=np.uint64)
        held = C.c_void_p()
        _check(lib().spsp_prevalence_device(self._h, k, d_min, d_lo, d_hi, sk_off.ctypes.data, n, n_query, num, den, rows.ctypes.data,
                                            spectrum.ctypes.data, C.byref(held) if want_holders else None))
        rows = rows[:n_query if n_query else n]
        return (rows, spectrum, held.value) if want_holders else (rows, spectrum)

    def prevalence_files(self, paths, out_prefix, num, den, n_query=0, precision=6, rate=0.0):
        """spsp_prevalence_files: sketch files (the n_query queries first, or all versus all) -> <out_prefix>_prevalence.csv.gz,
        <out_prefix>_spectrum.csv.gz and (rows, spectrum).  rate: as compare_files (0.0, a rate, or "auto")"""
        n = len(paths)
        arr, _alive = _paths_array(paths)
        rows, spec = C.c_void_p(), C.c_void_p()
        _check(lib().spsp_prevalence_files(self._h, arr, n, n_query, precision, num, den, out_prefix.encode(), 0, _rate_arg(rate),
                                           C.byref(rows), C.byref(spec)))
        n_rows = n_query if n_query else n
        return (np.frombuffer(_take(rows, n_rows * PREVALENCE_ROW_DTYPE.itemsize), dtype=PREVALENCE_ROW_DTYPE).copy(),
                np.frombuffer(_take(spec, (n - n_query + 1) * 8), dtype=np.uint64).copy())

    def select_device(self, k, d_min, d_lo, d_hi, sk_off, n, h_min, h_max, merged=False, n_query=0):
        """spsp_keys_select_device: the keys whose number of holders among the references lies in [h_min, h_max], over concatenated
        sorted key arrays on the device -> (d_minimizer, d_kmer_lo, d_kmer_hi or None, sk_off np.uint64): every row sketch's own,
        order kept (n_rows + 1 offsets), or merged=True the distinct keys of the references' union, sorted, as one sketch (two
        offsets) -- in arrays the context owns, valid until the next select call but one"""
        sk_off = np.ascontiguousarray(sk_off, dtype=np.uint64)
        if len(sk_off) != n + 1:
            raise ValueError("select_device: n + 1 sketch offsets")
        o_mn, o_lo, o_hi = C.c_void_p(), C.c_void_p(), C.c_void_p()
        out = np.zeros(2 if merged else max(n_query if n_query else n, 1) + 1, dtype=np.uint64)
        _check(lib().spsp_keys_select_device(self._h, k, d_min, d_lo, d_hi, sk_off.ctypes.data, n, n_query, h_min, h_max, 1 if merged else 0,
                                             C.byref(o_mn), C.byref(o_lo), C.byref(o_hi), out.ctypes.data))
        return o_mn.value, o_lo.value, o_hi.value, out

    def accumulation_device(self, k, d_min, d_lo, d_hi, sk_off, n, orders, want_curves=False):
        """spsp_accumulation_device: the pan and core curves of the sketches 0 .. n-1 over concatenated sorted key arrays on the
        device, for the given orders (P x n, every one a permutation of 0 .. n-1: accumulation_orders' or the caller's own) ->
        rows (ACCUMULATION_ROW_DTYPE array, row j-1 is step j) [, pan, core: np.uint64[P, n], every order's curves]"""
        sk_off = np.ascontiguousarray(sk_off, dtype=np.uint64)
        if len(sk_off) != n + 1:
            raise ValueError("accumulation_device: n + 1 sketch offsets")
        orders = np.ascontiguousarray(orders, dtype=np.uint32)
        if orders.ndim == 1:
            orders = orders.reshape(1, -1)
        if orders.ndim != 2 or orders.shape[1] != n:
            raise ValueError("accumulation_device: orders are P x n")
        P = orders.shape[0]
        rows = np.zeros(max(n, 1), dtype=ACCUMULATION_ROW_DTYPE)
        pan = np.zeros((P, n), dtype=np.uint64) if want_curves else None
        core = np.zeros((P, n), dtype=np.uint64) if want_curves else None
        _check(lib().spsp_accumulation_device(self._h, k, d_min, d_lo, d_hi, sk_off.ctypes.data, n, orders.ctypes.data if orders.size else rows.ctypes.data,
                                              P, rows.ctypes.data, pan.ctypes.data if want_curves and pan.size else None,
                                              core.ctypes.data if want_curves and core.size else None))
        rows = rows[:n]
        return (rows, pan, core) if want_curves else rows

    def accumulation_files(self, paths, prefix, orders=100, seed=1, precision=6, rate=0.0):
        """spsp_accumulation_files: sketch files -> <prefix>_accumulation.csv.gz and the rows; the curves are taken over `orders`
        orders, accumulation_orders(n, orders, seed).  rate: as compare_files (0.0, a rate, or "auto")"""
        n = len(paths)
        arr, _alive = _paths_array(paths)
        rows = C.c_void_p()
        _check(lib().spsp_accumulation_files(self._h, arr, n, orders, seed, precision, prefix.encode(), 0, _rate_arg(rate), C.byref(rows)))
        return np.frombuffer(_take(rows, n * ACCUMULATION_ROW_DTYPE.itemsize), dtype=ACCUMULATION_ROW_DTYPE).copy()

    def groups_device(self, k, d_min, d_lo, d_hi, sk_off, n, group, n_groups, num, den, onum=0, oden=1, want_markers=False):
        """spsp_groups_device: per group of the labelled sketches 0 .. n-1 (concatenated sorted key arrays on the device) the distinct
        keys present, core (held by ceil(num * size / den) members or more), exclusive (no holder outside) and marker (core, and at
        most floor(onum * (n - size) / oden) holders outside), and per sketch its own keys of the last three kinds ->
        (rows GROUP_ROW_DTYPE[n_groups], members GROUP_MEMBER_ROW_DTYPE[n]) [, (d_minimizer, d_kmer_lo, d_kmer_hi or None, marker_off
        np.uint64[n_groups + 1]): the groups' marker keys as sketches back to back in arrays the context owns, valid until the next
        groups call]"""
        sk_off = np.ascontiguousarray(sk_off, dtype=np.uint64)
        if len(sk_off) != n + 1:
            raise ValueError("groups_device: n + 1 sketch offsets")
        group = np.ascontiguousarray(group, dtype=np.uint32)
        if len(group) != n:
            raise ValueError("groups_device: one label per sketch")
        rows = np.zeros(max(n_groups, 1), dtype=GROUP_ROW_DTYPE)
        members = np.zeros(max(n, 1), dtype=GROUP_MEMBER_ROW_DTYPE)
        moff = np.zeros(max(n_groups, 0) + 1, dtype=np.uint64)
        o_mn, o_lo, o_hi = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().spsp_groups_device(self._h, k, d_min, d_lo, d_hi, sk_off.ctypes.data, n, group.ctypes.data if n else rows.ctypes.data, n_groups, num, den,
                                        onum, oden, rows.ctypes.data, members.ctypes.data, 1 if want_markers else 0, C.byref(o_mn), C.byref(o_lo),
                                        C.byref(o_hi), moff.ctypes.data))
        rows, members = rows[:n_groups], members[:n]
        return (rows, members, (o_mn.value, o_lo.value, o_hi.value, moff)) if want_markers else (rows, members)

    def groups_files(self, paths, prefix, labels, num, den, onum=0, oden=1, markers=False, precision=6, rate=0.0):
        """spsp_groups_files: sketch files and a labels file (one label per line, in the files' order) -> <prefix>_groups.csv.gz,
        <prefix>_members.csv.gz and, markers=True, <prefix>_markers_<c>.gz per group with the list <prefix>_markers.txt ->
        (rows, members).  rate: as compare_files (0.0, a rate, or "auto")"""
        n = len(paths)
        arr, _alive = _paths_array(paths)
        rows, members, G = C.c_void_p(), C.c_void_p(), C.c_uint32()
        _check(lib().spsp_groups_files(self._h, arr, n, str(labels).encode(), precision, num, den, onum, oden, 1 if markers else 0, prefix.encode(), 0,
                                       _rate_arg(rate), C.byref(rows), C.byref(members), C.byref(G)))
        return (np.frombuffer(_take(rows, G.value * GROUP_ROW_DTYPE.itemsize), dtype=GROUP_ROW_DTYPE).copy(),
                np.frombuffer(_take(members, n * GROUP_MEMBER_ROW_DTYPE.itemsize), dtype=GROUP_MEMBER_ROW_DTYPE).copy())

    def classify_index_device(self, k, d_min, d_lo, d_hi, sk_off, n_ref):
        """spsp_classify_index_device: the index of the references 0 .. n_ref-1 (concatenated sorted key arrays on the device, which
        must stay as they are while the index is in use), kept in the context until its next prevalence, select, accumulation,
        groups or index call"""
        sk_off = np.ascontiguousarray(sk_off, dtype=np.uint64)
        if len(sk_off) != n_ref + 1:
            raise ValueError("classify_index_device: n_ref + 1 sketch offsets")
        self._cf_n_ref = None
        _check(lib().spsp_classify_index_device(self._h, k, d_min, d_lo, d_hi, sk_off.ctypes.data, n_ref))
        self._cf_n_ref = n_ref

    def classify_device(self, d_min, d_lo, d_hi, rec_off, top=1, min_keys=1, num=0, den=1):
        """spsp_classify_device: the records whose distinct keys sit at [rec_off[r], rec_off[r + 1]) of key arrays on the device,
        against the context's index -> (records CLASSIFY_RECORD_DTYPE[n] with length 0, hits CLASSIFY_HIT_DTYPE[n, top])"""
        rec_off = np.ascontiguousarray(rec_off, dtype=np.uint64)
        if len(rec_off) < 1:
            raise ValueError("classify_device: n_records + 1 record offsets")
        n = len(rec_off) - 1
        records = np.zeros(max(n, 1), dtype=CLASSIFY_RECORD_DTYPE)
        hits = np.zeros((max(n, 1), max(top, 1)), dtype=CLASSIFY_HIT_DTYPE)
        _check(lib().spsp_classify_device(self._h, d_min, d_lo, d_hi, rec_off.ctypes.data, n, top, min_keys, num, den, records.ctypes.data, hits.ctypes.data))
        return records[:n], hits[:n]

    def classify_stage_ms(self):
        """spsp_classify_stage_ms: with timing_enable() on, the milliseconds of the classify calls' launches since the last read ->
        dict(probe, route, wave_form, workgroup_form); tally and selection are one kernel in each form"""
        ms = (C.c_double * 4)()
        _check(lib().spsp_classify_stage_ms(self._h, ms))
        return dict(zip(("probe", "route", "wave_form", "workgroup_form"), ms))

    def records_union_device(self, k, a_min, a_lo, a_hi, a_off, b_min, b_lo, b_hi, b_off):
        """spsp_records_union_device: per record the union of two sorted key lists on the device (a_hi / b_hi: None for k <= 32;
        a_off / b_off: n + 1 offsets each, which need not start at 0) -> (d_min, d_lo, d_hi, off): the context's arrays, valid
        until its next union call, and np.uint64[n + 1] offsets from 0"""
        a_off = np.ascontiguousarray(a_off, dtype=np.uint64)
        b_off = np.ascontiguousarray(b_off, dtype=np.uint64)
        if len(a_off) < 1 or len(a_off) != len(b_off):
            raise ValueError("records_union_device: n + 1 offsets on either side")
        n = len(a_off) - 1
        off = np.zeros(n + 1, dtype=np.uint64)
        o_mn, o_lo, o_hi = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().spsp_records_union_device(self._h, k, a_min, a_lo, a_hi, a_off.ctypes.data, b_min, b_lo, b_hi, b_off.ctypes.data, n, C.byref(o_mn),
                                               C.byref(o_lo), C.byref(o_hi), off.ctypes.data))
        return o_mn.value, o_lo.value, o_hi.value, off

    def union_stage_ms(self):
        """spsp_union_stage_ms: with timing_enable() on, the milliseconds of the union calls' launches since the last read ->
        dict(flags, scan, offsets, write)"""
        ms = (C.c_double * 4)()
        _check(lib().spsp_union_stage_ms(self._h, ms))
        return dict(zip(("flags", "scan", "offsets", "write"), ms))

    union_plan = staticmethod(union_plan)
    pairs_names = staticmethod(pairs_names)

    def _record_files(self, name, head, rest, outs, extract, gz, mates_path, split, window, window_call, default_call, smooth=0, segments=None, segments_min=1, raw=False):
        """the ladder classify_files and taxonomy_files share: the mode's checks, then spsp_<name>_files, _extract, _paired, _split
        or _windows.  head: (ctx, paths, n_ref, records_path), behind which the mates' path goes; rest: the pass's own arguments up
        to rate; outs: the rows' outputs, the count last; default_call: the word a windowed run calls by where window_call is None"""
        who = name + "_files"
        entry = lambda suffix: getattr(lib(), "spsp_" + who + suffix)
        refs = [C.byref(o) for o in outs]
        mates = None if mates_path is None else str(mates_path).encode()
        gz = 1 if gz else 0
        kept, out_bytes = C.c_uint64(), C.c_uint64()
        self._cf_n_ref = None
        if window is not None:
            if extract is not None or split is not None or mates_path is not None:
                raise ValueError("%s: window is not taken with extract, split or mates_path" % who)
            first, n_rec, seg, n_seg, mos = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64(), C.c_void_p()
            common = (*head, *rest, window, (window_call or default_call).encode(), *refs, C.byref(first), C.byref(n_rec), C.byref(seg), C.byref(n_seg), C.byref(mos))
            changed, written, text_bytes = C.c_uint64(), C.c_uint64(), C.c_uint64()
            raw_b, raw_e, bed_bytes = C.c_void_p(), C.c_void_p(), C.c_uint64()
            if raw:
                if not 0 <= smooth <= 0x7FFFFFFF or not 0 <= segments_min < 1 << 64:
                    raise ValueError("%s: smooth is 0 .. 2147483647, segments_min is not negative" % who)
                _check(entry("_raw")(*common, smooth, None if segments is None else segments.encode(), segments_min, gz, C.byref(changed), C.byref(written),
                                     C.byref(text_bytes), 1, C.byref(raw_b), C.byref(raw_e), C.byref(bed_bytes)))
            elif smooth or segments is not None or segments_min != 1:
                if not 0 <= smooth <= 0x7FFFFFFF or not 0 <= segments_min < 1 << 64:
                    raise ValueError("%s: smooth is 0 .. 2147483647, segments_min is not negative" % who)
                _check(entry("_segments")(*common, smooth, None if segments is None else segments.encode(), segments_min, gz, C.byref(changed), C.byref(written),
                                          C.byref(text_bytes)))
            else:
                _check(entry("_windows")(*common))
            self.last_windows = _windows_result(first, n_rec.value, seg, n_seg.value, mos)
            self.last_windows.update(changed=changed.value, written=written.value, bytes_out=text_bytes.value)
            if raw:
                n_seg = len(self.last_windows["segments"])
                self.last_windows.update(raw_begin=np.frombuffer(_take(raw_b, n_seg * 8), dtype=np.uint64).copy(),
                                         raw_end=np.frombuffer(_take(raw_e, n_seg * 8), dtype=np.uint64).copy(), bed_bytes=bed_bytes.value)
        elif window_call is not None or smooth or segments is not None or raw:
            raise ValueError("%s: window_call, smooth, segments and raw need window" % who)
        elif split is not None:
            if extract is not None:
                raise ValueError("%s: split writes every record and extract one subset: one of the two" % who)
            _check(entry("_split")(*head, mates, *rest, split.encode(), gz, *refs, C.byref(kept), C.byref(out_bytes)))
            self.last_split = {"bins": kept.value, "records": outs[-1].value, "bytes_out": out_bytes.value}
        elif mates_path is not None:
            _check(entry("_paired")(*head, mates, *rest, None if extract is None else extract.encode(), gz, *refs, C.byref(kept), C.byref(out_bytes)))
        elif extract is not None:
            _check(entry("_extract")(*head, *rest, *refs, extract.encode(), gz, C.byref(kept), C.byref(out_bytes)))
        else:
            _check(entry("")(*head, *rest, *refs))
        if extract is not None:
            self.last_extract = {"n_kept": kept.value, "bytes_out": out_bytes.value}

    def classify_files(self, paths, records_path, prefix, top=1, min_keys=1, num=0, den=1, precision=6, rate=0.0, extract=None, gz=True, mates_path=None,
                       split=None, window=None, window_call=None, smooth=0, segments=None, segments_min=1, raw=False):
        """spsp_classify_files: the sketch files of the references and a FASTA / FASTQ file of records (gzip or plain) ->
        <prefix>_classify.csv.gz, <prefix>_classify_summary.csv.gz and (records, hits[n, top]).  rate: as compare_files (0.0, a
        rate, or "auto"); sketches of different rates need one.  extract: a word (matched, unmatched, best=<j>, listed=<j>) --
        spsp_classify_files_extract: the records it names are written to <prefix>_extract.fa or .fq (".gz" appended when gz) as
        well; self.last_extract = dict(n_kept, bytes_out).  mates_path: the second file of paired reads -- spsp_classify_files_paired:
        record p of the two files is one pair, classified by the keys of both mates, and extract writes <prefix>_extract_1.* and
        <prefix>_extract_2.*.  split: the word `best` -- spsp_classify_files_split: every record goes to <prefix>_split_<j>.fa or .fq
        of its rank-1 match (or _split_unmatched.*; with mates_path _1 and _2 files), <prefix>_split.csv.gz lists them;
        self.last_split = dict(bins, records, bytes_out).  Not together with extract.  window: a width -- spsp_classify_files_windows:
        every record is cut into windows of that many bases, the returned rows are the WINDOWS', <prefix>_segments.csv.gz and
        <prefix>_mosaic.csv.gz take the per-record CSVs' place, and self.last_windows = dict(first_win, segments, mosaic);
        window_call: the call word (best).  Not together with extract, split or mates_path.  smooth: q -- with window
        (spsp_classify_files_segments), a run of at most q windows between two longer runs of one call takes that call.  segments: a
        word (all, called, none, call=<b>, not=<b>, major, minor) -- the segments it names of at least segments_min bases are written
        as <prefix>_segments.fa (".gz" appended when gz), one FASTA record <name>:<begin + 1>-<end> each; last_windows gains changed
        (windows the smoothing changed), written (segments) and bytes_out (the text's bytes).  raw: with window
        (spsp_classify_files_raw), the segments' raw intervals -- positions among the sequence characters of the records file's own
        records, N and lower case counted -- are made on the device and written as <prefix>_segments.bed (".gz" appended when gz);
        last_windows gains raw_begin, raw_end (one per segment) and bed_bytes"""
        arr, _alive = _paths_array(paths)
        recs, hits, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        self._record_files("classify", (self._h, arr, len(paths), str(records_path).encode()), (top, min_keys, num, den, precision, prefix.encode(), 0, _rate_arg(rate)),
                           (recs, hits, n), extract, gz, mates_path, split, window, window_call, "best", smooth, segments, segments_min, raw)
        return (np.frombuffer(_take(recs, n.value * CLASSIFY_RECORD_DTYPE.itemsize), dtype=CLASSIFY_RECORD_DTYPE).copy(),
                np.frombuffer(_take(hits, n.value * top * CLASSIFY_HIT_DTYPE.itemsize), dtype=CLASSIFY_HIT_DTYPE).copy().reshape(n.value, top))

    def records_extents_device(self, d_text, n_text):
        """spsp_records_extents_device: a FASTA / FASTQ text in HBM (16-byte aligned) -> (d_begin, n_rec): the context's uint64
        array of n_rec + 1 record starts, valid until the next extents call or the next extract call that makes its own"""
        d, n = C.c_void_p(), C.c_uint32()
        _check(lib().spsp_records_extents_device(self._h, d_text, n_text, C.byref(d), C.byref(n)))
        return d.value, n.value

    def records_extract_device(self, d_text, n_text, keep, d_begin=None, n_rec=None):
        """spsp_records_extract_device: the records of the text in HBM with keep[r] != 0, back to back -> (np.uint8 array,
        n_kept).  d_begin: the starts on the device (records_extents_device) or None: they are made in the call, for len(keep)
        records.  Only the kept bytes cross to the host"""
        keep = np.ascontiguousarray(keep, dtype=np.uint8)
        if n_rec is None:
            n_rec = len(keep)
        if len(keep) != n_rec:
            raise ValueError("records_extract_device: one flag per record")
        out, n_out, n_kept = C.c_void_p(), C.c_uint64(), C.c_uint64()
        _check(lib().spsp_records_extract_device(self._h, d_text, n_text, d_begin, n_rec, keep.ctypes.data if n_rec else None, C.byref(out), C.byref(n_out),
                                                 C.byref(n_kept)))
        return self.to_host(out.value, n_out.value, np.uint8), n_kept.value

    def records_split_device(self, d_text, n_text, bins, n_bins, d_begin=None, n_rec=None):
        """spsp_records_split_device: every record of the text in HBM in the slice of its bin (SPLIT_DROP: nowhere) -> (np.uint8
        array, bin_off: np.uint64[n_bins + 1], bin_records: np.uint64[n_bins]).  d_begin: the starts on the device
        (records_extents_device) or None: they are made in the call, for len(bins) records.  Every kept byte crosses to the host once"""
        bins = np.ascontiguousarray(bins, dtype=np.uint32)
        if n_rec is None:
            n_rec = len(bins)
        if len(bins) != n_rec:
            raise ValueError("records_split_device: one bin per record")
        room = n_bins if 0 < n_bins <= 1 << 24 else 0      # (an n_bins the call refuses gets no arrays to fill)
        off, rec = np.zeros(room + 1, dtype=np.uint64), np.zeros(max(room, 1), dtype=np.uint64)
        out, n_out = C.c_void_p(), C.c_uint64()
        _check(lib().spsp_records_split_device(self._h, d_text, n_text, d_begin, n_rec, bins.ctypes.data if n_rec else None, n_bins, C.byref(out), C.byref(n_out),
                                               off.ctypes.data, rec.ctypes.data))
        return self.to_host(out.value, n_out.value, np.uint8), off, rec[:n_bins]

    def records_windows_device(self, d_bases, n_bases, d_rec_off, n_rec, k, window, packed=False):
        """spsp_records_windows_device: the cleaned bases of a text in HBM (ASCII, or with packed the 2-bit words of
        SPSP_SCAN_PACKED_INPUT) and the records' base offsets on the device -> (d_out, n_out, d_win_off, first_win: np.uint32[n_rec + 1],
        n_windows): the windows' bases back to back in the same form and their offsets, both the context's until its next windows call"""
        first = np.zeros(n_rec + 1, dtype=np.uint32)
        out, n_out, off, n_win = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
        _check(lib().spsp_records_windows_device(self._h, d_bases, n_bases, d_rec_off, n_rec, k, window, 1 if packed else 0, C.byref(out), C.byref(n_out),
                                                 C.byref(off), first.ctypes.data, C.byref(n_win)))
        return out.value, n_out.value, off.value, first, n_win.value

    def windows_stage_ms(self):
        """spsp_windows_stage_ms: with timing_enable() on, the milliseconds of the windows calls' launches since the last read ->
        dict(count, offsets, copy)"""
        ms = (C.c_double * 3)()
        _check(lib().spsp_windows_stage_ms(self._h, ms))
        return dict(zip(("count", "offsets", "copy"), ms))

    windows_plan = staticmethod(windows_plan)

    def segments_write_device(self, d_bases, n_bases, src, length, headers, hdr_off, packed=False):
        """spsp_segments_write_device: the cleaned bases of a text in HBM (ASCII, or with packed the 2-bit words) and per segment its
        global base offset, its bases and its header (headers[hdr_off[i]:hdr_off[i + 1]]) -> (d_out, n_out): the FASTA text in the
        context's buffer, queued on its stream (to_host waits), valid until the context's next call"""
        src = np.ascontiguousarray(src, dtype=np.uint64)
        length = np.ascontiguousarray(length, dtype=np.uint64)
        hdr_off = np.ascontiguousarray(hdr_off, dtype=np.uint64)
        blob = np.frombuffer(bytes(headers), dtype=np.uint8)
        if len(src) != len(length) or len(hdr_off) != len(src) + 1 or int(hdr_off[-1]) > len(blob):
            raise ValueError("segments_write_device: one source and one length per segment, n_seg + 1 header offsets inside the headers")
        out, n_out = C.c_void_p(), C.c_uint64()
        _check(lib().spsp_segments_write_device(self._h, d_bases, n_bases, 1 if packed else 0, src.ctypes.data if len(src) else None,
                                                length.ctypes.data if len(src) else None, blob.ctypes.data if len(blob) else None, hdr_off.ctypes.data, len(src),
                                                C.byref(out), C.byref(n_out)))
        return out.value, n_out.value

    def segments_stage_ms(self):
        """spsp_segments_stage_ms: with timing_enable() on, the milliseconds of the segments' writes since the last read -> dict(write)"""
        ms = (C.c_double * 1)()
        _check(lib().spsp_segments_stage_ms(self._h, ms))
        return {"write": ms[0]}

    segments_plan = staticmethod(segments_plan)

    def records_lift_device(self, d_text, n_text, n_bases, base, n_rec=None):
        """spsp_records_lift_device: the raw text in HBM (16-byte aligned), the kept bases the ingest counted for it, and GLOBAL
        kept-base indices (rec_off[r] + p, non-decreasing) -> (raw: np.uint64[n_q], rec: np.uint32[n_q], raw_length:
        np.uint64[n_rec], every record's sequence characters).  n_rec: the records the ingest counted, which is raw_length's room
        (the lengths need it before the call's one wait); without it records_extents_device counts them first, one more call and
        wait.  self.last_lift_records: the records the pass itself counted"""
        base = _lift_base(base)
        n_q = len(base)
        raw, rec = np.zeros(max(n_q, 1), dtype=np.uint64), np.zeros(max(n_q, 1), dtype=np.uint32)
        if n_rec is None:
            n_rec = self.records_extents_device(d_text, n_text)[1]
        raw_length = np.zeros(max(n_rec, 1), dtype=np.uint64)
        room = C.c_uint32(n_rec)
        _check(lib().spsp_records_lift_device(self._h, d_text, n_text, n_bases, base.ctypes.data if n_q else None, n_q, raw.ctypes.data, rec.ctypes.data,
                                              raw_length.ctypes.data, C.byref(room)))
        self.last_lift_records = room.value
        return raw[:n_q], rec[:n_q], raw_length[:n_rec]

    def lift_stage_ms(self):
        """spsp_lift_stage_ms: with timing_enable() on, the milliseconds of the lift calls' launches since the last read ->
        dict(count, scan, answer)"""
        ms = (C.c_double * 3)()
        _check(lib().spsp_lift_stage_ms(self._h, ms))
        return dict(zip(("count", "scan", "answer"), ms))

    lift_plan = staticmethod(lift_plan)

    def split_stage_ms(self):
        """spsp_split_stage_ms: with timing_enable() on, the milliseconds of the split calls' launches since the last read ->
        dict(starts, runs, order, offsets, copy)"""
        ms = (C.c_double * 5)()
        _check(lib().spsp_split_stage_ms(self._h, ms))
        return dict(zip(("starts", "runs", "order", "offsets", "copy"), ms))

    def extract_stage_ms(self):
        """spsp_extract_stage_ms: with timing_enable() on, the milliseconds of the extract calls' launches since the last read ->
        dict(starts, offsets, copy)"""
        ms = (C.c_double * 3)()
        _check(lib().spsp_extract_stage_ms(self._h, ms))
        return dict(zip(("starts", "offsets", "copy"), ms))

    def taxonomy_index_device(self, parent, ref_node, want_key_nodes=False):
        """spsp_taxonomy_index_device: a tree (parents in preorder) and the references' nodes attached to the context's index
        (classify_index_device first); it ends with that index [-> d_key_nodes: the device address of the context's uint32 array
        of node(x) per index entry, valid until the next attach or index call]"""
        parent = np.ascontiguousarray(parent, dtype=np.uint32)
        ref_node = np.ascontiguousarray(ref_node, dtype=np.uint32)
        d = C.c_void_p()
        _check(lib().spsp_taxonomy_index_device(self._h, parent.ctypes.data if len(parent) else None, len(parent), ref_node.ctypes.data if len(ref_node) else None,
                                                len(ref_node), C.byref(d) if want_key_nodes else None))
        return d.value if want_key_nodes else None

    def taxonomy_device(self, d_min, d_lo, d_hi, rec_off, min_keys=1, num=0, den=1):
        """spsp_taxonomy_device: the records whose distinct keys sit at [rec_off[r], rec_off[r + 1]) of key arrays on the device,
        against the taxonomy of the context's index -> records TAXONOMY_RECORD_DTYPE[n] with length 0"""
        rec_off = np.ascontiguousarray(rec_off, dtype=np.uint64)
        if len(rec_off) < 1:
            raise ValueError("taxonomy_device: n_records + 1 record offsets")
        n = len(rec_off) - 1
        records = np.zeros(max(n, 1), dtype=TAXONOMY_RECORD_DTYPE)
        _check(lib().spsp_taxonomy_device(self._h, d_min, d_lo, d_hi, rec_off.ctypes.data, n, min_keys, num, den, records.ctypes.data))
        return records[:n]

    def taxonomy_stage_ms(self):
        """spsp_taxonomy_stage_ms: with timing_enable() on, the milliseconds of the taxonomy calls' launches since the last read ->
        dict(probe, route, wave_form, workgroup_form)"""
        ms = (C.c_double * 4)()
        _check(lib().spsp_taxonomy_stage_ms(self._h, ms))
        return dict(zip(("probe", "route", "wave_form", "workgroup_form"), ms))

    def taxonomy_files(self, paths, records_path, lineages_path, prefix, min_keys=1, num=0, den=1, precision=6, rate=0.0, extract=None, gz=True, mates_path=None,
                       split=None, window=None, window_call=None, smooth=0, segments=None, segments_min=1, raw=False):
        """spsp_taxonomy_files: the sketch files of the references, a FASTA / FASTQ file of records (gzip or plain) and the lineage
        file of the references -> <prefix>_taxonomy.csv.gz, <prefix>_taxonomy_report.csv.gz and the records.  rate: as
        classify_files (0.0, a rate, or "auto"); sketches of different rates need one.  extract: a word (classified, unclassified,
        taxon=<t>, clade=<t>) -- spsp_taxonomy_files_extract: the records it names are written to <prefix>_extract.fa or .fq (".gz"
        appended when gz) as well; self.last_extract = dict(n_kept, bytes_out).  mates_path: as classify_files
        (spsp_taxonomy_files_paired).  split: a word (taxon, depth=<d>) -- spsp_taxonomy_files_split: every record goes to
        <prefix>_split_<t>.fa or .fq of its node (or _split_unclassified.*), as classify_files; self.last_split.  window,
        window_call (taxon, depth=<d>): spsp_taxonomy_files_windows, as classify_files; self.last_windows.  smooth, segments,
        segments_min: spsp_taxonomy_files_segments, as classify_files (<b> is a node's number).  raw: spsp_taxonomy_files_raw, as
        classify_files"""
        arr, _alive = _paths_array(paths)
        recs, n = C.c_void_p(), C.c_uint64()
        self._record_files("taxonomy", (self._h, arr, len(paths), str(records_path).encode()),
                           (str(lineages_path).encode(), min_keys, num, den, precision, prefix.encode(), 0, _rate_arg(rate)), (recs, n), extract, gz, mates_path, split,
                           window, window_call, "taxon", smooth, segments, segments_min, raw)
        return np.frombuffer(_take(recs, n.value * TAXONOMY_RECORD_DTYPE.itemsize), dtype=TAXONOMY_RECORD_DTYPE).copy()

    def depth_begin(self):
        """spsp_depth_begin_device: one cleared counter per distinct key of the context's index (classify_index_device); they end
        with that index"""
        _check(lib().spsp_depth_begin_device(self._h))

    def depth_add(self, d_min, d_lo, d_hi, first, n_keys):
        """spsp_depth_add_device: the keys of whole records (distinct per record, any order) at entries [first, first + n_keys) of
        key arrays on the device, counted into the index's counters.  Only queues: the arrays must stay until the next read"""
        _check(lib().spsp_depth_add_device(self._h, d_min, d_lo, d_hi, first, n_keys))

    def depth_read(self, min_count=1, want_counts=False):
        """spsp_depth_read_device: -> (rows DEPTH_ROW_DTYPE[n_ref], totals: a DEPTH_TOTALS_DTYPE scalar [, d_counts: the device
        address of the context's uint32 array of c per index entry, valid until the next read, begin or index call]).  n_ref: the
        references of the index this context built last.  The counters stay: it may be called again"""
        n_ref = getattr(self, "_cf_n_ref", None)
        rows = np.zeros(65535 if n_ref is None else max(n_ref, 1), dtype=DEPTH_ROW_DTYPE)   # (the library writes as many rows as ITS index has references)
        totals = np.zeros(1, dtype=DEPTH_TOTALS_DTYPE)
        d = C.c_void_p()
        _check(lib().spsp_depth_read_device(self._h, min_count, rows.ctypes.data, totals.ctypes.data, C.byref(d) if want_counts else None))
        rows = rows[:n_ref or 0]
        return (rows, totals[0], d.value) if want_counts else (rows, totals[0])

    def depth_stage_ms(self):
        """spsp_depth_stage_ms: with timing_enable() on, the milliseconds of the depth calls' launches since the last read ->
        dict(add, entry, reduce)"""
        ms = (C.c_double * 3)()
        _check(lib().spsp_depth_stage_ms(self._h, ms))
        return dict(zip(("add", "entry", "reduce"), ms))

    def depth_files(self, paths, reads_paths, prefix, min_count=1, precision=6, rate=0.0):
        """spsp_depth_files: the sketch files of the references and one or more FASTA / FASTQ files of reads (gzip or plain) ->
        <prefix>_depth.csv.gz and (rows, totals).  rate: as classify_files (0.0, a rate, or "auto"); sketches of different rates need one"""
        arr, _alive = _paths_array(paths)
        reads, _alive2 = _paths_array([str(r) for r in reads_paths])
        rows = C.c_void_p()
        totals = np.zeros(1, dtype=DEPTH_TOTALS_DTYPE)
        self._cf_n_ref = None
        _check(lib().spsp_depth_files(self._h, arr, len(paths), reads, len(reads_paths), min_count, precision, prefix.encode(), 0, _rate_arg(rate),
                                      C.byref(rows), totals.ctypes.data))
        return np.frombuffer(_take(rows, len(paths) * DEPTH_ROW_DTYPE.itemsize), dtype=DEPTH_ROW_DTYPE).copy(), totals[0]

    def profile_read(self, min_count=1, min_keys=1, max_rounds=0, want_assigned=False):
        """spsp_profile_device: the greedy rounds on the counters of depth_begin / depth_add -> (rows PROFILE_ROW_DTYPE, one per
        round, totals: a PROFILE_TOTALS_DTYPE scalar [, d_assigned: the device address of the context's byte array parallel to the
        index's key arrays, 1 where the entry's key was assigned to the entry's reference; valid until the next profile, begin or
        index call]).  The counters stay: it may be called again, and a depth_read before or after it answers as without it"""
        n_ref = getattr(self, "_cf_n_ref", None)
        rows = np.zeros(65535 if n_ref is None else max(n_ref, 1), dtype=PROFILE_ROW_DTYPE)   # (the library writes at most as many rows as ITS index has references)
        totals = np.zeros(1, dtype=PROFILE_TOTALS_DTYPE)
        d, n = C.c_void_p(), C.c_uint64()
        _check(lib().spsp_profile_device(self._h, min_count, min_keys, max_rounds, rows.ctypes.data, C.byref(n), totals.ctypes.data,
                                         C.byref(d) if want_assigned else None))
        rows = rows[:n.value].copy()
        return (rows, totals[0], d.value) if want_assigned else (rows, totals[0])

    def profile_stage_ms(self):
        """spsp_profile_stage_ms and spsp_profile_counts: with timing_enable() on, the milliseconds of the profile calls' launches since
        the last read -> dict(start, picks, walks, reduction), and what the last call did -> rounds (queued), rows, waits (of the host)"""
        ms = (C.c_double * 4)()
        counts = (C.c_uint32 * 3)()
        _check(lib().spsp_profile_stage_ms(self._h, ms))
        _check(lib().spsp_profile_counts(self._h, counts))
        out = dict(zip(("start", "picks", "walks", "reduction"), ms))
        out.update(zip(("rounds", "rows", "waits"), (int(c) for c in counts)))
        return out

    def profile_files(self, paths, reads_paths, prefix, min_count=1, min_keys=1, max_rounds=0, precision=6, rate=0.0):
        """spsp_profile_files: as depth_files, and one profile behind the read -> <prefix>_depth.csv.gz, <prefix>_profile.csv.gz and
        (depth rows, depth totals, profile rows, profile totals)"""
        arr, _alive = _paths_array(paths)
        reads, _alive2 = _paths_array([str(r) for r in reads_paths])
        rows, prows, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        totals = np.zeros(1, dtype=DEPTH_TOTALS_DTYPE)
        ptotals = np.zeros(1, dtype=PROFILE_TOTALS_DTYPE)
        self._cf_n_ref = None
        _check(lib().spsp_profile_files(self._h, arr, len(paths), reads, len(reads_paths), min_count, min_keys, max_rounds, precision, prefix.encode(), 0,
                                        _rate_arg(rate), C.byref(rows), totals.ctypes.data, C.byref(prows), C.byref(n), ptotals.ctypes.data))
        return (np.frombuffer(_take(rows, len(paths) * DEPTH_ROW_DTYPE.itemsize), dtype=DEPTH_ROW_DTYPE).copy(), totals[0],
                np.frombuffer(_take(prows, n.value * PROFILE_ROW_DTYPE.itemsize), dtype=PROFILE_ROW_DTYPE).copy(), ptotals[0])

    def select_files(self, paths, prefix, what, each=False, n_query=0, rate=None):
        """spsp_select_files: sketch files (the n_query queries first, or none) -> the keys in the band `what` (select_band's words)
        as sketch files: <prefix>_select.gz, or each=True one <prefix>_<i>_<basename> per row sketch and the list
        <prefix>_select.txt -> (keys in, keys written).  rate: None or 0.0 (the headers' rates, which must agree), a rate, or "auto" for the coarsest of the files'"""
        n = len(paths)
        arr, _alive = _paths_array(paths)
        k_in, k_out = C.c_uint64(), C.c_uint64()
        _check(lib().spsp_select_files(self._h, arr, n, n_query, str(what).encode(), 1 if each else 0, prefix.encode(), 0,
                                       _rate_arg(0.0 if rate is None else rate), C.byref(k_in), C.byref(k_out)))
        return k_in.value, k_out.value
