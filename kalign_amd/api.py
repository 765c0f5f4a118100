"""ctypes binding of include/kalign_amd.h (host mirror of the reference's dispatcher seam).

Function names follow the reference: msa_tree() stands where create_msa_tree()
(lib/src/aln_run.c:43) is called, pairwise_batch() where anchor_consistency_build loops over
pairwise_align_map() (lib/src/anchor_consistency.c:246-267).
"""
import ctypes as C
import os
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

FLAG_DEBUG_ROWS = 1
FLAG_TIMING = 2
FLAG_DEVICE_GAPS = 4
FLAG_KEEP_CONSISTENCY = 8
FLAG_EXACT_CONFIDENCE = 16
FLAG_LEAF_PROFILES = 32
ERR_ROWS_STRIDE = 3             # KA_ERR_ROWS_STRIDE: the row buffer is too narrow, the width is reported


class KalignAmdError(RuntimeError):
    pass


class TaskRec(C.Structure):
    """ka_task_rec (include/kalign_amd.h)"""
    _fields_ = [
        ("a", C.c_int), ("b", C.c_int), ("c", C.c_int),
        ("len_a", C.c_int), ("len_b", C.c_int),
        ("nsip_a", C.c_int), ("nsip_b", C.c_int),
        ("plen", C.c_int), ("kind", C.c_int), ("swapped", C.c_int),
        ("meet", C.c_int), ("transition", C.c_int), ("path_off", C.c_int),
        ("gap_scale", C.c_float), ("subm_off", C.c_float),
        ("score", C.c_float), ("confidence", C.c_float),
        ("prof_hash", C.c_uint64), ("fhash", C.c_uint64), ("bhash", C.c_uint64),
    ]


# ka_dist_fn of include/kalign_amd.h
DIST_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int))

EXPORTS = ["ka_tree_profile_dev", "ka_tree_reserve_profile_dev", "ka_tree_build_consistency_part",
           "ka_tree_consistency_part_range", "ka_tree_consistency_maps_dev", "ka_debug_set_hooks", "ka_debug_reload_env", "ka_debug_plan", "ka_debug_ctx_plan", "ka_debug_kmeans_level", "ka_debug_kmeans_host", "ka_ctx_fallback_runs", "ka_ctx_arena_bytes", "ka_ctx_helped_tasks", "ka_ctx_create", "ka_ctx_destroy", "ka_ctx_set_stream", "ka_ctx_set_shared", "ka_last_error", "ka_abi_version",
           "ka_msa_tree", "ka_tree_upload", "ka_tree_run", "ka_tree_refine", "ka_tree_refine_trees", "ka_debug_refine_marks", "ka_tree_sync", "ka_tree_paths_size",
           "ka_tree_download", "ka_tree_get_profile", "ka_tree_get_timing", "ka_debug_trace", "ka_tree_cells", "ka_tree_kernel_ms", "ka_tree_launch_ms",
           "ka_pairwise_batch", "ka_pairwise_kernel_ms", "ka_tree_build_consistency", "ka_tree_get_consistency",
           "ka_tree_run_tasks", "ka_tree_reset", "ka_tree_node_len", "ka_tree_set_profile", "ka_tree_download_tasks", "ka_weave_gaps",
           "ka_tree_node_cols_size", "ka_tree_get_node_cols", "ka_tree_set_node_cols", "ka_bpm_batch",
           "ka_tree_aligned_rows", "ka_guide_tree", "ka_guide_tree_from",
           "ka_aln_guide_tree", "ka_run_encoded", "ka_run_encoded_refine", "ka_tree_plan_tasks", "ka_tree_run_planned",
           "ka_dist_unique_id", "ka_dist_create", "ka_dist_destroy", "ka_dist_plan_subtrees", "ka_dist_plan", "ka_dist_get_plan",
           "ka_dist_consistency", "ka_dist_tree_run", "ka_dist_paths_size", "ka_dist_download", "ka_dist_last_ms", "ka_dist_retries",
           "ka_dist_loopback_new", "ka_dist_loopback_free", "ka_dist_create_loopback",
           "ka_guide_last_bisect_ms", "ka_device_count", "ka_multi_create", "ka_multi_destroy", "ka_multi_world", "ka_multi_runs", "ka_multi_last_error",
           "ka_multi_consistency", "ka_multi_tree_run", "ka_multi_paths_size", "ka_multi_download", "ka_multi_ctx", "ka_multi_adopt",
           "ka_tree_adopt_alignment", "ka_ens_create", "ka_ens_destroy", "ka_ens_add_member", "ka_ens_score_rows", "ka_ens_consensus",
           "ka_ens_confidence", "ka_ens_stats", "ka_ens_table_size", "ka_ens_table_write", "ka_ens_table_image", "ka_ens_open_table",
           "ka_ens_open_table_image", "ka_ens_n_runs", "ka_ens_table_stats", "ka_poar_check_image", "ka_ens_merge", "ka_ens_select", "ka_cmp_create", "ka_cmp_destroy", "ka_cmp_set_mask", "ka_cmp_score",
           "ka_cmp_score_batch", "ka_cmp_stats",
           "ka_cmp_fam_check", "ka_cmp_fam_create", "ka_cmp_fam_destroy", "ka_cmp_fam_set_masks", "ka_cmp_fam_score", "ka_cmp_fam_stats",
           "ka_cmp_detail", "ka_cmp_fam_detail", "ka_cmp_detail_stats", "ka_cmp_fam_detail_stats", "ka_calibration",
           "ka_ens_fam_check", "ka_ens_fam_create", "ka_ens_fam_destroy", "ka_ens_fam_add_member", "ka_ens_fam_score_members", "ka_ens_fam_score",
           "ka_ens_fam_consensus", "ka_ens_fam_rows_size", "ka_ens_fam_rows", "ka_ens_fam_confidence", "ka_ens_fam_stats",
           "ka_debug_ens_fam_consensus_host",
           "ka_sum_fam_check", "ka_sum_fam_create", "ka_sum_fam_destroy", "ka_sum_fam_columns", "ka_sum_fam_summary", "ka_sum_fam_consensus",
           "ka_sum_fam_keep", "ka_sum_fam_compact", "ka_sum_fam_rows_size", "ka_sum_fam_rows", "ka_sum_fam_stats",
           "ka_sum_fam_identity_entries", "ka_sum_fam_identity", "ka_sum_fam_identity_stats",
           "ka_sum_fam_gaps", "ka_sum_fam_gap_values", "ka_sum_fam_ungapped_size", "ka_sum_fam_ungapped", "ka_sum_fam_gap_stats",
           "ka_guide_forest_from", "ka_guide_forest", "ka_aln_guide_forest", "ka_run_encoded_batch", "ka_batch_rows_size", "ka_batch_rows",
           "ka_batch_stats", "ka_batch_refine_stats",
           "ka_in_tables", "ka_in_detect", "ka_in_order", "ka_in_fam_check", "ka_in_fam_create", "ka_in_fam_destroy", "ka_in_fam_sequences",
           "ka_in_fam_families", "ka_in_fam_order", "ka_in_fam_size", "ka_in_fam_encoded", "ka_in_fam_run", "ka_in_fam_rows_size",
           "ka_in_fam_rows", "ka_in_fam_stats",
           "ka_cod_table", "ka_cod_fam_check", "ka_cod_fam_create", "ka_cod_fam_destroy", "ka_cod_fam_sequences", "ka_cod_fam_protein_size",
           "ka_cod_fam_protein", "ka_cod_fam_run", "ka_cod_fam_back", "ka_cod_fam_rows_size", "ka_cod_fam_rows",
           "ka_cod_fam_protein_rows_size", "ka_cod_fam_protein_rows", "ka_cod_fam_stats",
           "ka_out_pp_char", "ka_out_fam_check", "ka_out_fam_text_sizes", "ka_out_fam_create", "ka_out_fam_destroy", "ka_out_fam_fasta_size", "ka_out_fam_fasta",
           "ka_out_fam_clustal_size", "ka_out_fam_clustal", "ka_out_fam_msf_records", "ka_out_fam_msf_size", "ka_out_fam_msf",
           "ka_out_fam_stockholm_size", "ka_out_fam_stockholm", "ka_out_fam_stats"]


def lib_path():
    return os.path.join(_HERE, "libkalign_amd.so")


_lib = None


def load_library():
    """Loads the HIP library.  Raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    p = lib_path()
    if not os.path.exists(p):
        raise KalignAmdError("%s not built: run `make -C kalign_amd/csrc` or __graft_entry__.build()" % p)
    L = C.CDLL(p)
    vp = C.c_void_p
    L.ka_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.ka_ctx_destroy.argtypes = [vp]
    L.ka_ctx_destroy.restype = None
    L.ka_ctx_set_stream.argtypes = [vp, vp]
    L.ka_ctx_set_shared.argtypes = [vp, C.c_int]
    L.ka_last_error.restype = C.c_char_p
    L.ka_debug_set_hooks.argtypes = [vp, C.c_int]
    L.ka_debug_reload_env.argtypes = [vp]
    L.ka_debug_plan.argtypes = [C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, C.c_int, vp, vp]
    L.ka_debug_ctx_plan.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp]
    L.ka_tree_profile_dev.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_int)]
    L.ka_tree_reserve_profile_dev.argtypes = [vp, C.c_int, C.c_int, C.POINTER(vp)]
    L.ka_tree_build_consistency_part.argtypes = [vp, C.c_int, C.c_float, C.c_int, C.c_int]
    L.ka_tree_consistency_part_range.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    L.ka_tree_consistency_maps_dev.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_longlong)]
    L.ka_ctx_fallback_runs.argtypes = [vp]
    L.ka_ctx_arena_bytes.argtypes = [vp]
    L.ka_ctx_arena_bytes.restype = C.c_longlong
    L.ka_ctx_helped_tasks.argtypes = [vp]
    L.ka_ctx_helped_tasks.restype = C.c_longlong
    L.ka_debug_kmeans_level.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_int)]
    L.ka_debug_kmeans_host.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    L.ka_abi_version.restype = C.c_int
    L.ka_msa_tree.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, vp, C.c_int,
                              C.POINTER(TaskRec), vp, C.c_longlong, vp]
    L.ka_tree_upload.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, vp, C.c_int]
    L.ka_tree_run.argtypes = [vp]
    L.ka_tree_refine.argtypes = [vp, C.c_int, vp]
    L.ka_tree_refine_trees.argtypes = [vp, C.c_int, vp, vp, vp, C.POINTER(C.c_int)]
    L.ka_debug_refine_marks.argtypes = [C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp, C.POINTER(C.c_int)]
    L.ka_tree_sync.argtypes = [vp]
    L.ka_tree_paths_size.argtypes = [vp]
    L.ka_tree_paths_size.restype = C.c_longlong
    L.ka_tree_download.argtypes = [vp, C.POINTER(TaskRec), vp, C.c_longlong, vp]
    L.ka_tree_get_profile.argtypes = [vp, C.c_int, vp, C.c_longlong]
    L.ka_tree_get_timing.argtypes = [vp, vp]
    L.ka_debug_trace.argtypes = [vp, vp]
    L.ka_pairwise_kernel_ms.argtypes = [vp]
    L.ka_pairwise_kernel_ms.restype = C.c_float
    L.ka_tree_cells.argtypes = [vp]
    L.ka_tree_cells.restype = C.c_double
    L.ka_tree_kernel_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_int)]
    L.ka_tree_launch_ms.argtypes = [vp, vp, C.c_int]
    L.ka_tree_run_tasks.argtypes = [vp, vp, C.c_int]
    L.ka_tree_plan_tasks.argtypes = [vp, vp, C.c_int]
    L.ka_tree_run_planned.argtypes = [vp]
    L.ka_dist_unique_id.argtypes = [vp]
    L.ka_dist_create.argtypes = [vp, C.c_int, C.c_int, vp, C.POINTER(vp)]
    L.ka_dist_destroy.argtypes = [vp]
    L.ka_dist_destroy.restype = None
    L.ka_dist_plan_subtrees.argtypes = [C.c_int, vp, C.c_int, vp, C.c_int, vp, vp, C.POINTER(C.c_int)]
    L.ka_dist_plan.argtypes = [vp]
    L.ka_dist_get_plan.argtypes = [vp, vp, vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.ka_dist_consistency.argtypes = [vp, C.c_int, C.c_float]
    L.ka_dist_tree_run.argtypes = [vp]
    L.ka_dist_paths_size.argtypes = [vp]
    L.ka_dist_paths_size.restype = C.c_longlong
    L.ka_dist_download.argtypes = [vp, vp, vp, C.c_longlong, C.POINTER(C.c_longlong)]
    L.ka_dist_last_ms.argtypes = [vp]
    L.ka_dist_last_ms.restype = C.c_double
    L.ka_dist_retries.argtypes = [vp]
    L.ka_device_count.argtypes = []
    L.ka_guide_last_bisect_ms.argtypes = [vp]
    L.ka_guide_last_bisect_ms.restype = C.c_double
    L.ka_multi_create.argtypes = [C.c_int, vp, C.c_int, C.POINTER(vp)]
    L.ka_multi_destroy.argtypes = [vp]
    L.ka_multi_destroy.restype = None
    L.ka_multi_world.argtypes = [vp]
    L.ka_multi_runs.argtypes = [vp]
    L.ka_multi_runs.restype = C.c_longlong
    L.ka_multi_last_error.argtypes = []
    L.ka_multi_last_error.restype = C.c_char_p
    L.ka_multi_consistency.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_float, vp, vp]
    L.ka_multi_tree_run.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_float]
    L.ka_multi_paths_size.argtypes = [vp]
    L.ka_multi_paths_size.restype = C.c_longlong
    L.ka_multi_download.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp, C.c_longlong, vp]
    L.ka_multi_ctx.argtypes = [vp, C.c_int]
    L.ka_multi_ctx.restype = vp
    L.ka_multi_adopt.argtypes = [vp, vp, vp]
    L.ka_tree_adopt_alignment.argtypes = [vp, vp, vp]
    L.ka_dist_loopback_new.argtypes = [C.c_int]
    L.ka_dist_loopback_new.restype = vp
    L.ka_dist_loopback_free.argtypes = [vp]
    L.ka_dist_loopback_free.restype = None
    L.ka_dist_create_loopback.argtypes = [vp, C.c_int, C.c_int, vp, C.POINTER(vp)]
    L.ka_tree_reset.argtypes = [vp]
    L.ka_tree_node_len.argtypes = [vp, C.c_int]
    L.ka_tree_set_profile.argtypes = [vp, C.c_int, vp, C.c_int]
    L.ka_tree_node_cols_size.argtypes = [vp, C.c_int]
    L.ka_tree_node_cols_size.restype = C.c_longlong
    L.ka_tree_get_node_cols.argtypes = [vp, C.c_int, vp]
    L.ka_tree_set_node_cols.argtypes = [vp, C.c_int, vp]
    L.ka_tree_download_tasks.argtypes = [vp, vp, C.c_int, C.POINTER(TaskRec), vp, C.c_longlong, C.POINTER(C.c_longlong)]
    L.ka_weave_gaps.argtypes = [C.c_int, vp, C.c_int, C.POINTER(TaskRec), vp, vp]
    L.ka_bpm_batch.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, C.c_int, vp]
    L.ka_tree_build_consistency.argtypes = [vp, C.c_int, C.c_float]
    L.ka_tree_aligned_rows.argtypes = [vp, vp, C.c_ubyte, vp, C.c_longlong, vp]
    L.ka_run_encoded.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_float, C.c_int, vp, C.c_int,
                                 C.c_ubyte, vp, C.c_longlong, vp]
    L.ka_run_encoded_refine.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_float, C.c_int, vp, C.c_int, C.c_int,
                                        C.c_ubyte, vp, C.c_longlong, vp]
    L.ka_aln_guide_tree.argtypes = [vp, C.c_int, vp, C.c_longlong, C.c_int, C.c_ubyte, vp, vp, vp]
    L.ka_guide_tree.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp]
    L.ka_guide_tree_from.argtypes = [C.c_int, vp, DIST_FN, vp, C.c_int, vp, vp, vp]
    L.ka_guide_forest_from.argtypes = [C.c_int, vp, vp, DIST_FN, vp, C.c_int, vp, vp, C.POINTER(C.c_int), vp]
    L.ka_guide_forest.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, C.POINTER(C.c_int), vp]
    L.ka_aln_guide_forest.argtypes = [vp, C.c_int, vp, vp, C.c_longlong, vp, C.c_ubyte, vp, vp, vp]
    L.ka_run_encoded_batch.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_float, C.c_int, vp, C.c_int,
                                       C.c_int, C.c_ubyte, vp]
    L.ka_batch_rows_size.argtypes = [vp]
    L.ka_batch_rows_size.restype = C.c_longlong
    L.ka_batch_rows.argtypes = [vp, vp, C.c_longlong]
    L.ka_batch_stats.argtypes = [vp, vp]
    L.ka_batch_refine_stats.argtypes = [vp, C.c_int, vp, vp, vp]
    L.ka_tree_get_consistency.argtypes = [vp, vp, vp]
    L.ka_pairwise_batch.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, C.c_int, vp,
                                    C.c_float, C.c_float, C.c_float, vp, vp, vp]
    L.ka_ens_create.argtypes = [vp, C.c_int, vp, C.c_int, C.POINTER(vp)]
    L.ka_ens_destroy.argtypes = [vp]
    L.ka_ens_destroy.restype = None
    L.ka_ens_add_member.argtypes = [vp, C.c_int, vp, C.c_longlong, C.c_int]
    L.ka_ens_score_rows.argtypes = [vp, vp, C.c_longlong, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_double)]
    L.ka_ens_consensus.argtypes = [vp, C.c_int, vp, vp, C.c_longlong, C.POINTER(C.c_int)]
    L.ka_ens_confidence.argtypes = [vp, vp, C.c_longlong, C.c_int, vp, vp]
    L.ka_ens_stats.argtypes = [vp, vp, vp, vp]
    L.ka_ens_table_size.argtypes = [vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    L.ka_ens_table_write.argtypes = [vp, C.c_char_p]
    L.ka_ens_table_image.argtypes = [vp, vp, C.c_longlong]
    L.ka_ens_open_table.argtypes = [vp, C.c_int, vp, C.c_char_p, C.POINTER(vp)]
    L.ka_ens_open_table_image.argtypes = [vp, C.c_int, vp, vp, C.c_longlong, C.POINTER(vp)]
    L.ka_ens_n_runs.argtypes = [vp]
    L.ka_ens_table_stats.argtypes = [vp, vp]
    L.ka_ens_merge.argtypes = [vp, vp, C.POINTER(vp)]
    L.ka_ens_select.argtypes = [vp, vp, C.c_int, C.POINTER(vp)]
    L.ka_poar_check_image.argtypes = [vp, C.c_longlong, C.c_int, vp, C.POINTER(C.c_int), C.POINTER(C.c_longlong)]
    L.ka_cmp_create.argtypes = [vp, C.c_int, vp, vp, C.c_longlong, C.c_int, C.POINTER(vp)]
    L.ka_cmp_destroy.argtypes = [vp]
    L.ka_cmp_destroy.restype = None
    L.ka_cmp_set_mask.argtypes = [vp, C.c_float, vp, C.c_int]
    L.ka_cmp_score.argtypes = [vp, vp, C.c_longlong, C.c_int, vp, vp, vp]
    L.ka_cmp_score_batch.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp]
    L.ka_cmp_stats.argtypes = [vp, vp]
    L.ka_cmp_fam_check.argtypes = [C.c_int, vp, vp, vp, vp]
    L.ka_cmp_fam_create.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.POINTER(vp)]
    L.ka_cmp_fam_destroy.argtypes = [vp]
    L.ka_cmp_fam_destroy.restype = None
    L.ka_cmp_fam_set_masks.argtypes = [vp, vp, vp, vp]
    L.ka_cmp_fam_score.argtypes = [vp, vp, vp, vp, vp, vp]
    L.ka_cmp_fam_stats.argtypes = [vp, vp]
    L.ka_cmp_detail.argtypes = [vp, vp, C.c_longlong, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.ka_cmp_fam_detail.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.ka_cmp_detail_stats.argtypes = [vp, vp]
    L.ka_cmp_fam_detail_stats.argtypes = [vp, vp]
    L.ka_calibration.argtypes = [C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, vp]
    L.ka_ens_fam_check.argtypes = [C.c_int, vp, vp, vp, vp]
    L.ka_ens_fam_create.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.POINTER(vp)]
    L.ka_ens_fam_destroy.argtypes = [vp]
    L.ka_ens_fam_destroy.restype = None
    L.ka_ens_fam_add_member.argtypes = [vp, C.c_int, vp, vp]
    L.ka_ens_fam_score_members.argtypes = [vp, vp, vp]
    L.ka_ens_fam_score.argtypes = [vp, vp, vp, vp, vp]
    L.ka_ens_fam_consensus.argtypes = [vp, vp, vp, C.c_int, vp]
    L.ka_ens_fam_rows_size.argtypes = [vp]
    L.ka_ens_fam_rows_size.restype = C.c_longlong
    L.ka_ens_fam_rows.argtypes = [vp, vp, C.c_longlong]
    L.ka_ens_fam_confidence.argtypes = [vp, vp, vp, vp, vp]
    L.ka_ens_fam_stats.argtypes = [vp, vp]
    L.ka_debug_ens_fam_consensus_host.argtypes = [C.c_int, vp, vp, vp, vp, vp, C.c_int, vp, vp, C.c_longlong]
    L.ka_sum_fam_check.argtypes = [C.c_int, vp, vp, vp]
    L.ka_sum_fam_create.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, C.POINTER(vp)]
    L.ka_sum_fam_destroy.argtypes = [vp]
    L.ka_sum_fam_destroy.restype = None
    L.ka_sum_fam_columns.argtypes = [vp, vp, vp, vp, vp, vp]
    L.ka_sum_fam_summary.argtypes = [vp, vp, vp]
    L.ka_sum_fam_consensus.argtypes = [vp, vp, vp, vp]
    L.ka_sum_fam_keep.argtypes = [vp, vp, vp, vp, vp, vp]
    L.ka_sum_fam_compact.argtypes = [vp, vp, vp, vp, vp]
    L.ka_sum_fam_rows_size.argtypes = [vp]
    L.ka_sum_fam_rows_size.restype = C.c_longlong
    L.ka_sum_fam_rows.argtypes = [vp, vp, C.c_longlong]
    L.ka_sum_fam_stats.argtypes = [vp, vp]
    L.ka_sum_fam_identity_entries.argtypes = [C.c_int, vp]
    L.ka_sum_fam_identity_entries.restype = C.c_longlong
    L.ka_sum_fam_identity.argtypes = [vp, vp, vp, vp]
    L.ka_sum_fam_identity_stats.argtypes = [vp, vp]
    L.ka_sum_fam_gaps.argtypes = [vp, vp, vp, vp]
    L.ka_sum_fam_gap_values.argtypes = [C.c_int, vp, vp]
    L.ka_sum_fam_ungapped_size.argtypes = [vp]
    L.ka_sum_fam_ungapped_size.restype = C.c_longlong
    L.ka_sum_fam_ungapped.argtypes = [vp, vp, C.c_longlong, vp]
    L.ka_sum_fam_gap_stats.argtypes = [vp, vp]
    L.ka_in_tables.argtypes = [vp]
    L.ka_in_detect.argtypes = [vp, C.POINTER(C.c_int)]
    L.ka_in_order.argtypes = [C.c_int, vp, vp, vp, vp, vp]
    L.ka_in_fam_check.argtypes = [C.c_int, vp, vp, C.c_longlong]
    L.ka_in_fam_create.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, C.POINTER(vp)]
    L.ka_in_fam_destroy.argtypes = [vp]
    L.ka_in_fam_destroy.restype = None
    L.ka_in_fam_sequences.argtypes = [vp, vp]
    L.ka_in_fam_families.argtypes = [vp, vp, vp]
    L.ka_in_fam_order.argtypes = [vp, vp]
    L.ka_in_fam_size.argtypes = [vp]
    L.ka_in_fam_size.restype = C.c_longlong
    L.ka_in_fam_encoded.argtypes = [vp, vp, vp, vp, vp, vp]
    L.ka_in_fam_run.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_ubyte]
    L.ka_in_fam_rows_size.argtypes = [vp]
    L.ka_in_fam_rows_size.restype = C.c_longlong
    L.ka_in_fam_rows.argtypes = [vp, vp, C.c_longlong, vp]
    L.ka_in_fam_stats.argtypes = [vp, vp]
    L.ka_cod_table.argtypes = [vp]
    L.ka_cod_fam_check.argtypes = [C.c_int, vp, vp, C.c_longlong]
    L.ka_cod_fam_create.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, C.POINTER(vp)]
    L.ka_cod_fam_destroy.argtypes = [vp]
    L.ka_cod_fam_destroy.restype = None
    L.ka_cod_fam_sequences.argtypes = [vp, vp]
    L.ka_cod_fam_protein_size.argtypes = [vp]
    L.ka_cod_fam_protein_size.restype = C.c_longlong
    L.ka_cod_fam_protein.argtypes = [vp, vp, vp]
    L.ka_cod_fam_run.argtypes = [vp, vp, vp, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_ubyte]
    L.ka_cod_fam_back.argtypes = [vp, vp, C.c_longlong, vp, C.c_ubyte]
    for name in ("ka_cod_fam_rows", "ka_cod_fam_protein_rows"):
        getattr(L, name + "_size").argtypes = [vp]
        getattr(L, name + "_size").restype = C.c_longlong
        getattr(L, name).argtypes = [vp, vp, C.c_longlong, vp]
    L.ka_cod_fam_stats.argtypes = [vp, vp]
    L.ka_out_pp_char.argtypes = [C.c_float]
    L.ka_out_fam_check.argtypes = [C.c_int, vp, vp, vp, vp, vp]
    L.ka_out_fam_text_sizes.argtypes = [C.c_int, vp, vp, vp, C.c_int, C.c_int, vp]
    L.ka_out_fam_create.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, vp, vp, C.POINTER(vp)]
    L.ka_out_fam_destroy.argtypes = [vp]
    L.ka_out_fam_destroy.restype = None
    L.ka_out_fam_fasta_size.argtypes = [vp, C.c_int]
    L.ka_out_fam_fasta_size.restype = C.c_longlong
    L.ka_out_fam_fasta.argtypes = [vp, C.c_int, vp, C.c_longlong, vp]
    L.ka_out_fam_clustal_size.argtypes = [vp, C.c_char_p]
    L.ka_out_fam_clustal_size.restype = C.c_longlong
    L.ka_out_fam_clustal.argtypes = [vp, C.c_char_p, vp, C.c_longlong, vp]
    L.ka_out_fam_msf_records.argtypes = [vp, vp, vp]
    L.ka_out_fam_msf_size.argtypes = [vp, vp, vp, vp, C.c_char_p]
    L.ka_out_fam_msf_size.restype = C.c_longlong
    L.ka_out_fam_msf.argtypes = [vp, vp, vp, vp, C.c_char_p, vp, C.c_longlong, vp]
    L.ka_out_fam_stockholm_size.argtypes = [vp, C.c_int, C.c_int]
    L.ka_out_fam_stockholm_size.restype = C.c_longlong
    L.ka_out_fam_stockholm.argtypes = [vp, vp, vp, vp, C.c_longlong, vp]
    L.ka_out_fam_stats.argtypes = [vp, vp]
    _lib = L
    return L


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _flatten(codes):
    lens = np.array([len(c) for c in codes], np.int32)
    off = np.zeros(len(codes), np.int32)
    off[1:] = np.cumsum(lens)[:-1]
    flat = np.ascontiguousarray(np.concatenate(codes), np.uint8)
    return flat, off, lens


class Context:
    """One GPU context (ka_ctx)."""

    def __init__(self, device=0, stream=None, shared=False):
        """shared=True: other streams / processes use the GPU at the same time (ka_ctx_set_shared)."""
        self.L = load_library()
        h = C.c_void_p()
        if self.L.ka_ctx_create(device, C.byref(h)):
            raise KalignAmdError(self.L.ka_last_error().decode())
        self.h = h
        if stream is not None:
            self.L.ka_ctx_set_stream(self.h, C.c_void_p(stream))
        if shared:
            self.L.ka_ctx_set_shared(self.h, 1)
        self._job = None

    @classmethod
    def borrowed(cls, handle, job=None):
        """A view of a context somebody else owns (Multi.ctx): close() does not destroy it."""
        self = cls.__new__(cls)
        self.L = load_library()
        self.h = C.c_void_p(handle) if not isinstance(handle, C.c_void_p) else handle
        self._job = job
        self._borrowed = True
        return self

    def close(self):
        # ensembles and comparers borrow this context's stream: they go first
        for e in list(getattr(self, "_children", ())):
            e.close()
        if getattr(self, "h", None):
            if not getattr(self, "_borrowed", False):
                self.L.ka_ctx_destroy(self.h)
            self.h = None

    def adopt_alignment(self, recs, gaps):
        """ka_tree_adopt_alignment: this context (same uploaded job) takes over an alignment made elsewhere."""
        arr = (TaskRec * len(recs))(*recs)
        flat = np.ascontiguousarray(np.concatenate([np.asarray(g, np.int32) for g in gaps]), np.int32)
        self._chk(self.L.ka_tree_adopt_alignment(self.h, arr, _ptr(flat)))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def debug_set_hooks(self, hooks):
        """tests only: ka_debug_set_hooks (KA_DEBUG_SMALL_ARENAS = 1, KA_DEBUG_STARVE_ROOT_JOIN = 2, KA_DEBUG_STARVE_REFINE_MEMBER = 4, KA_DEBUG_CHAIN_FIRST = 8, KA_DEBUG_POISON_ARENAS = 16)"""
        self._chk(self.L.ka_debug_set_hooks(self.h, int(hooks)))

    def reload_env(self):
        """tools / tests: the KA_* environment switches are read once at context creation; read them again"""
        self._chk(self.L.ka_debug_reload_env(self.h))

    def debug_plan(self, n_cus=256):
        """ka_debug_ctx_plan: the launch plan this context holds, flattened like debug_plan()'s (n_cus only sizes the first buffer)"""
        return _flat_plan(self.L, self._job["ntasks"], int(n_cus), lambda *out: self.L.ka_debug_ctx_plan(self.h, *out))

    def fallback_runs(self):
        return int(self.L.ka_ctx_fallback_runs(self.h))

    def arena_bytes(self):
        """device bytes in the profile, path and scratch arenas (ka_ctx_arena_bytes)"""
        return int(self.L.ka_ctx_arena_bytes(self.h))

    def helped_tasks(self):
        """queue tasks of the last run that workgroups of the chained launch took over (ka_ctx_helped_tasks)"""
        return int(self.L.ka_ctx_helped_tasks(self.h))

    def _chk(self, rc):
        if rc:
            raise KalignAmdError("rc=%d: %s" % (rc, self.L.ka_last_error().decode()))

    # ---- staged dispatcher -------------------------------------------------------------
    def tree_upload(self, codes, tasks, subm, scal, seq_distances=None, flags=0):
        flat, off, lens = _flatten(codes)
        tasks = np.ascontiguousarray(tasks, np.int32)
        sd = None if seq_distances is None else np.ascontiguousarray(seq_distances, np.float32)
        sub = np.ascontiguousarray(subm, np.float32).reshape(-1)
        sc = np.ascontiguousarray(scal, np.float32)
        self._chk(self.L.ka_tree_upload(self.h, len(codes), _ptr(flat), _ptr(off), _ptr(lens), _ptr(sd),
                                        len(tasks), _ptr(tasks), _ptr(sub), _ptr(sc), flags))
        self._job = dict(lens=lens, ntasks=len(tasks), n=len(codes))

    def tree_run(self):
        self._chk(self.L.ka_tree_run(self.h))

    def tree_refine(self, mode, conf_in=None):
        """refine_alignment (aln_refine.c:34-85) over the uploaded tree: mode 1 = all edges, 2 = edges whose
        first-pass confidence (conf_in; None: computed on the device) is at or below the median, 3 = inline
        refinement (create_msa_tree_inline_refine), 4 = the plain first pass, depth first (exact confidences)."""
        cf = None if conf_in is None else np.ascontiguousarray(conf_in, np.float32)
        if cf is not None and len(cf) != self._job["ntasks"]:
            raise KalignAmdError("tree_refine: one confidence per task")
        self._chk(self.L.ka_tree_refine(self.h, int(mode), None if cf is None else _ptr(cf)))

    def tree_refine_trees(self, mode, conf_in=None):
        """ka_tree_refine_trees: tree_refine with mode 2's median per tree of a forest job (tree_refine pools it over the
        job); on a job of one tree the same call.  Returns (tree_of[n_tasks], thr[n_trees]): the tree of every task, trees
        numbered by their root task, and every tree's threshold (zeros in the other modes)."""
        nt = self._job["ntasks"]
        cf = None if conf_in is None else np.ascontiguousarray(conf_in, np.float32)
        if cf is not None and len(cf) != nt:
            raise KalignAmdError("tree_refine_trees: one confidence per task")
        tree_of, thr, n = np.zeros(nt, np.int32), np.zeros(nt, np.float32), C.c_int(0)
        self._chk(self.L.ka_tree_refine_trees(self.h, int(mode), None if cf is None else _ptr(cf), _ptr(tree_of), _ptr(thr), C.byref(n)))
        return tree_of, thr[:n.value].copy()

    def tree_sync(self):
        self._chk(self.L.ka_tree_sync(self.h))

    def tree_kernel_ms(self):
        ms, n = C.c_float(0), C.c_int(0)
        self._chk(self.L.ka_tree_kernel_ms(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def tree_plan_tasks(self, task_ids):
        """the listed tasks as ONE planned run (queued / chained launches); None = the whole tree again"""
        if task_ids is None:
            self._chk(self.L.ka_tree_plan_tasks(self.h, None, 0))
        else:
            ids = np.ascontiguousarray(task_ids, np.int32)
            self._chk(self.L.ka_tree_plan_tasks(self.h, _ptr(ids), len(ids)))

    def tree_run_planned(self):
        self._chk(self.L.ka_tree_run_planned(self.h))

    def tree_launch_ms(self):
        """per-launch kernel times of the last run (KA_LAUNCH_EV=1 when the context was created / reload_env)"""
        out = np.zeros(96, np.float32)
        n = self.L.ka_tree_launch_ms(self.h, _ptr(out), 96)
        if n < 0:
            raise RuntimeError(self.L.ka_last_error().decode())
        return out[:n].tolist()

    def tree_cells(self):
        return self.L.ka_tree_cells(self.h)

    def tree_download(self, want_gaps=True):
        j = self._job
        self.tree_sync()
        cap = self.L.ka_tree_paths_size(self.h)
        recs = (TaskRec * j["ntasks"])()
        paths = np.zeros(max(int(cap), 1), np.int32)
        gaps = np.zeros(int(j["lens"].sum()) + j["n"], np.int32) if want_gaps else None
        self._chk(self.L.ka_tree_download(self.h, recs, _ptr(paths), cap, _ptr(gaps)))
        g = None
        if want_gaps:
            g, o = [], 0
            for n in j["lens"]:
                g.append(gaps[o:o + int(n) + 1].copy())
                o += int(n) + 1
        return recs, paths, g

    def tree_aligned_rows(self, letters, gap=b"-"):
        """finalise_alignment on the device: `letters` holds, per sequence, what to print for each residue (bytes,
        str or uint8 array); returns one bytes object per sequence, as long as the alignment of its tree."""
        j = self._job

        def as_u8(x):
            if isinstance(x, np.ndarray):
                return x.astype(np.uint8)
            return np.frombuffer(x.encode() if isinstance(x, str) else bytes(x), np.uint8)

        flat = np.ascontiguousarray(np.concatenate([as_u8(x) for x in letters]))
        if len(flat) != int(j["lens"].sum()) or any(len(x) != n for x, n in zip(letters, j["lens"])):
            raise KalignAmdError("letters do not match the uploaded sequences")
        alen = np.zeros(j["n"], np.int32)
        self._chk(self.L.ka_tree_aligned_rows(self.h, _ptr(flat), gap[0], None, 0, _ptr(alen)))   # size query
        stride = int(alen.max()) + 1
        rows = np.zeros((j["n"], stride), np.uint8)
        self._chk(self.L.ka_tree_aligned_rows(self.h, _ptr(flat), gap[0], _ptr(rows), stride, _ptr(alen)))
        assert all(rows[i, alen[i]] == 0 for i in range(j["n"]))
        return [rows[i, :alen[i]].tobytes() for i in range(j["n"])]

    def tree_timing(self):
        n = self._job["ntasks"]
        out = np.zeros(8 * n + 48 + 512, np.int64)
        self._chk(self.L.ka_tree_get_timing(self.h, _ptr(out)))
        self.root_levels = out[8 * n:8 * n + 48].reshape(16, 3)      # per recursion level of the root task: n, pass, meetup
        self.prof = out[8 * n + 48:].reshape(8, 8, 8)                 # KA_PROF builds: [level][wave][slot]
        return out[:8 * n].reshape(n, 8)

    def pairwise_kernel_ms(self):
        return float(self.L.ka_pairwise_kernel_ms(self.h))

    def debug_trace(self):
        out = np.zeros(64, np.int32)
        self._chk(self.L.ka_debug_trace(self.h, _ptr(out)))
        return out

    def tree_profile(self, node, max_cols):
        out = np.zeros(64 * (max_cols + 2), np.float32)
        self._chk(self.L.ka_tree_get_profile(self.h, node, _ptr(out), out.size))
        return out

    # ---- one-shot -----------------------------------------------------------------------
    # ---- partial runs (single-tree multi-GPU sharding, kalign_amd/dist.py:sharded_tree) ----
    def tree_run_tasks(self, task_ids):
        ids = np.ascontiguousarray(task_ids, np.int32)
        self._chk(self.L.ka_tree_run_tasks(self.h, _ptr(ids), len(ids)))

    def tree_reset(self):
        self._chk(self.L.ka_tree_reset(self.h))

    def tree_node_len(self, node):
        n = self.L.ka_tree_node_len(self.h, int(node))
        if n < 0:
            raise KalignAmdError("ka_tree_node_len failed")
        return n

    def tree_get_node(self, node):
        """State of an internal node as one float32 array: the merged profile [(plen+2)*64] followed, when the job
        has a consistency table, by the residue->column table of its members (ints viewed as float32)."""
        self.tree_sync()
        prof = self.tree_profile(node, self.tree_node_len(node))
        if self.L.ka_tree_get_consistency(self.h, None, None) > 0:
            n = int(self.L.ka_tree_node_cols_size(self.h, int(node)))
            cols = np.zeros(n, np.int32)
            self._chk(self.L.ka_tree_get_node_cols(self.h, int(node), _ptr(cols)))
            return np.concatenate([prof, cols.view(np.float32)])
        return prof

    def tree_set_node(self, node, state):
        state = np.ascontiguousarray(state, np.float32).reshape(-1)
        ncols = 0
        if self.L.ka_tree_get_consistency(self.h, None, None) > 0:
            ncols = int(self.L.ka_tree_node_cols_size(self.h, int(node)))
        prof = np.ascontiguousarray(state[:len(state) - ncols])
        self._chk(self.L.ka_tree_set_profile(self.h, int(node), _ptr(prof), len(prof) // 64 - 2))
        if ncols:
            cols = np.ascontiguousarray(state[len(state) - ncols:]).view(np.int32)
            self._chk(self.L.ka_tree_set_node_cols(self.h, int(node), _ptr(cols)))

    # ---- device-to-device hand-over (sharded trees; kalign_amd/dist.py wraps the pointers as torch tensors) ----
    def tree_profile_dev(self, node):
        """(device pointer, plen) of a node's merged profile: (plen+2)*64 float32 in this context's HBM"""
        ptr, plen = C.c_void_p(), C.c_int(0)
        self._chk(self.L.ka_tree_profile_dev(self.h, int(node), C.byref(ptr), C.byref(plen)))
        return ptr.value, plen.value

    def tree_reserve_profile_dev(self, node, plen):
        """room for an incoming profile of `plen` columns; returns the device pointer to fill before the parent runs"""
        ptr = C.c_void_p()
        self._chk(self.L.ka_tree_reserve_profile_dev(self.h, int(node), int(plen), C.byref(ptr)))
        return ptr.value

    def tree_node_cols(self, node):
        """residue -> column table of a node's members (None without a consistency table)"""
        if self.L.ka_tree_get_consistency(self.h, None, None) <= 0:
            return None
        n = int(self.L.ka_tree_node_cols_size(self.h, int(node)))
        cols = np.zeros(n, np.int32)
        self._chk(self.L.ka_tree_get_node_cols(self.h, int(node), _ptr(cols)))
        return cols

    def tree_set_node_cols(self, node, cols):
        cols = np.ascontiguousarray(cols, np.int32)
        self._chk(self.L.ka_tree_set_node_cols(self.h, int(node), _ptr(cols)))

    def tree_build_consistency_part(self, n_anchors, weight, part, nparts):
        """this rank's share of the N x K batch of a sharded consistency build (ka_tree_build_consistency_part)"""
        self._chk(self.L.ka_tree_build_consistency_part(self.h, int(n_anchors), float(weight), int(part), int(nparts)))

    def tree_consistency_part_range(self, part, nparts):
        lo, hi = C.c_longlong(0), C.c_longlong(0)
        self._chk(self.L.ka_tree_consistency_part_range(self.h, int(part), int(nparts), C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def tree_consistency_maps_dev(self):
        """(device pointer, number of int32) of the position-map table in HBM"""
        ptr, n = C.c_void_p(), C.c_longlong(0)
        self._chk(self.L.ka_tree_consistency_maps_dev(self.h, C.byref(ptr), C.byref(n)))
        return ptr.value, n.value

    # (the executor interface of kalign_amd.dist.sharded_consistency)
    def cons_build_part(self, n_anchors, weight, part, nparts):
        self.tree_build_consistency_part(n_anchors, weight, part, nparts)

    def cons_part_range(self, part, nparts):
        return self.tree_consistency_part_range(part, nparts)

    def cons_table(self):
        import torch
        from . import dist as kd
        if self.L.ka_tree_get_consistency(self.h, None, None) <= 0:
            return None
        ptr, n = self.tree_consistency_maps_dev()
        return kd.dev_tensor(ptr, n, torch.int32)

    def tree_download_tasks(self, task_ids):
        """(recs, paths) of the listed tasks; recs[i].path_off indexes `paths`."""
        ids = np.ascontiguousarray(task_ids, np.int32)
        recs = (TaskRec * max(len(ids), 1))()
        cap = int(self._job["lens"].sum()) * 2 * max(len(ids), 1) + 8 * len(ids) + 16
        cap = min(cap, (int(self._job["lens"].sum()) + 2) * (len(ids) + 1) + 16)
        paths = np.zeros(cap, np.int32)
        used = C.c_longlong(0)
        self._chk(self.L.ka_tree_download_tasks(self.h, _ptr(ids), len(ids), recs, _ptr(paths), cap, C.byref(used)))
        return list(recs)[:len(ids)], paths[:used.value]

    def tree_build_consistency(self, n_anchors=5, weight=2.0):
        """anchor_consistency_build: call between tree_upload and tree_run (the reference's default mode)."""
        self._chk(self.L.ka_tree_build_consistency(self.h, int(n_anchors), float(weight)))

    def tree_consistency(self):
        """(anchor_ids[K], maps[i][k]) or None when the job has no consistency table."""
        K = self.L.ka_tree_get_consistency(self.h, None, None)
        if K <= 0:
            return None
        lens = self._job["lens"]
        ids = np.full(max(len(lens), K), -1, np.int32)        # a forest job: K anchors per alignment
        flat = np.zeros(int(lens.sum()) * K, np.int32)
        self.L.ka_tree_get_consistency(self.h, _ptr(ids), _ptr(flat))
        ids = ids[ids >= 0]
        maps, o = [], 0
        for n in lens:
            row = []
            for _ in range(K):
                row.append(flat[o:o + int(n)].copy())
                o += int(n)
            maps.append(row)
        return ids, maps

    def msa_tree(self, codes, tasks, subm, scal, seq_distances=None, flags=0, n_anchors=0, weight=2.0):
        # like ka_msa_tree: the gap arrays are wanted, so let the device keep every residue's column
        self.tree_upload(codes, tasks, subm, scal, seq_distances, flags | FLAG_DEVICE_GAPS)
        if n_anchors > 0:
            self.tree_build_consistency(n_anchors, weight)
        self.tree_run()
        return self.tree_download()

    def pairwise_batch(self, codes, ia, ib, subm, gpo, gpe, tgpe):
        flat, off, lens = _flatten(codes)
        ia = np.ascontiguousarray(ia, np.int32)
        ib = np.ascontiguousarray(ib, np.int32)
        sizes = lens[ia].astype(np.int64) + lens[ib] + 3
        poff = np.zeros(len(ia), np.int64)
        poff[1:] = np.cumsum(sizes)[:-1]
        paths = np.zeros(int(sizes.sum()), np.int32)
        scores = np.zeros(len(ia), np.float32)
        sub = np.ascontiguousarray(subm, np.float32).reshape(-1)
        self._chk(self.L.ka_pairwise_batch(self.h, _ptr(flat), _ptr(off), _ptr(lens), len(codes),
                                           _ptr(ia), _ptr(ib), len(ia), _ptr(sub),
                                           float(gpo), float(gpe), float(tgpe), _ptr(paths), _ptr(poff), _ptr(scores)))
        return [paths[poff[k]:poff[k] + paths[poff[k]] + 2].copy() for k in range(len(ia))], scores


def _bpm_batch(self, codes, ia, ib):
    """calc_distance / bpm_block for a list of pairs (codes < 13): int32 distances."""
    flat, off, lens = _flatten(codes)
    ia = np.ascontiguousarray(ia, np.int32)
    ib = np.ascontiguousarray(ib, np.int32)
    out = np.zeros(len(ia), np.int32)
    self._chk(self.L.ka_bpm_batch(self.h, _ptr(flat), _ptr(off), _ptr(lens), len(codes), _ptr(ia), _ptr(ib), len(ia), _ptr(out)))
    return out


Context.bpm_batch = _bpm_batch


def _dm_scale(noise, n):
    if noise is None:
        return None
    noise = np.ascontiguousarray(noise, np.float32).reshape(-1)
    if len(noise) != n * min(32, n):
        raise KalignAmdError("dm_scale needs numseq * min(32, numseq) multipliers")
    return noise


def _guide_tree(self, codes, n_threads=1, dm_scale=None):
    """build_tree_kmeans with both distance batches on the device: (tasks[n-1, 3], seq_distances[n]).
    `codes` in the alphabet the reference builds its tree in (reduced protein alphabet / nucleotides);
    dm_scale: the multipliers of build_tree_kmeans_noisy, or None."""
    flat, off, lens = _flatten(codes)
    tasks = np.zeros((len(codes) - 1, 3), np.int32)
    sd = np.zeros(len(codes), np.float32)
    sc = _dm_scale(dm_scale, len(codes))
    self._chk(self.L.ka_guide_tree(self.h, len(codes), _ptr(flat), _ptr(off), _ptr(lens), int(n_threads), _ptr(sc), _ptr(tasks), _ptr(sd)))
    return tasks, sd


Context.guide_tree = _guide_tree


def _kmeans_level(self, dm, samples, sets, force_big=False):
    """tests only: ka_debug_kmeans_level -- ONE level of the device bisection as ka_kmeans_device launches it.
    dm[numrows, 32] float32, samples = the level's sample buffer (row indices), sets = [(start, n), ...] slices of it.
    Returns (per set: dict(score[tries], counts[tries, 2], lists[tries, 2, n] (sl / sr valid up to their counts),
    mind[tries, n], wmean[32], winner)), big) -- big: the <512, 512> shape ran."""
    dm = np.ascontiguousarray(dm, np.float32)
    samples = np.ascontiguousarray(samples, np.int32)
    sets = np.ascontiguousarray(sets, np.int32).reshape(-1, 2)
    if dm.ndim != 2 or dm.shape[1] != 32:
        raise KalignAmdError("dm needs 32 columns")
    tries = np.minimum(40, sets[:, 1]).astype(np.int64)
    per = tries * sets[:, 1]                                  # samples x candidates of every set
    before = np.concatenate([[0], np.cumsum(per)])
    cand0 = np.concatenate([[0], np.cumsum(tries)])
    score = np.zeros(int(cand0[-1]), np.float32)
    counts = np.zeros((int(cand0[-1]), 2), np.int32)
    lists = np.full(2 * int(before[-1]), -1, np.int32)
    mind = np.zeros(int(before[-1]), np.float32)
    wmean = np.zeros((len(sets), 32), np.float32)
    winner = np.zeros(len(sets), np.int32)
    big = C.c_int(0)
    self._chk(self.L.ka_debug_kmeans_level(self.h, _ptr(dm), dm.shape[0], _ptr(samples), len(samples), _ptr(sets), len(sets), int(bool(force_big)),
                                           _ptr(score), _ptr(counts), _ptr(lists), _ptr(mind), _ptr(wmean), _ptr(winner), C.byref(big)))
    out = []
    for k, (start, n) in enumerate(sets):
        t, b = int(tries[k]), int(before[k])
        out.append(dict(score=score[cand0[k]:cand0[k] + t], counts=counts[cand0[k]:cand0[k] + t],
                        lists=lists[2 * b:2 * b + 2 * t * n].reshape(t, 2, n), mind=mind[b:b + t * n].reshape(t, n),
                        wmean=wmean[k], winner=int(winner[k])))
    return out, bool(big.value)


Context.kmeans_level = _kmeans_level


def kmeans_host(dm, samples, seed_pick):
    """tests only: ka_debug_kmeans_host -- the host's split2 (ka_guide.cpp) on one set from one seed; no GPU needed.
    dict(score, counts[2], sl, sr, mind[n] (min(dl, dr) of the last iteration), wmean[32], iterations, parity_total /
    parity_last (samples decided by the index parity rule over all iterations / in the last one), degenerate)."""
    L = load_library()
    dm = np.ascontiguousarray(dm, np.float32)
    samples = np.ascontiguousarray(samples, np.int32)
    if dm.ndim != 2 or dm.shape[1] != 32:
        raise KalignAmdError("dm needs 32 columns")
    n = len(samples)
    score = np.zeros(1, np.float32)
    counts = np.zeros(2, np.int32)
    lists = np.full((2, n), -1, np.int32)
    mind = np.zeros(n, np.float32)
    wmean = np.zeros(32, np.float32)
    counters = np.zeros(4, np.int32)
    if L.ka_debug_kmeans_host(_ptr(dm), dm.shape[0], _ptr(samples), n, int(seed_pick), _ptr(score), _ptr(counts), _ptr(lists),
                              _ptr(mind), _ptr(wmean), _ptr(counters)):
        raise KalignAmdError(L.ka_last_error().decode())
    return dict(score=score[0], counts=counts, sl=lists[0, :counts[0]].copy(), sr=lists[1, :counts[1]].copy(), mind=mind, wmean=wmean,
                iterations=int(counters[0]), parity_total=int(counters[1]), parity_last=int(counters[2]), degenerate=bool(counters[3]))


def _aln_guide_tree(self, rows=None, n=None, gap=b"-", want_dm=False):
    """The guide tree of a realignment pass (compute_aln_pairwise_dist + build_tree_from_pairwise on the device):
    (tasks, seq_distances[, dm]).  rows: equal-length byte strings, or None for the rows the last
    tree_aligned_rows left in HBM (then n = number of sequences of that job)."""
    if rows is None:
        n = self._job["n"] if n is None else n
        flat, stride, alnlen = None, 0, 0
    else:
        n = len(rows)
        alnlen = len(rows[0])
        if any(len(r) != alnlen for r in rows):
            raise KalignAmdError("rows of one alignment have one length")
        flat = np.frombuffer(b"".join(bytes(r) for r in rows), np.uint8)
        stride = alnlen
    tasks = np.zeros((n - 1, 3), np.int32)
    sd = np.zeros(n, np.float32)
    dm = np.zeros((n, n), np.float32) if want_dm else None
    self._chk(self.L.ka_aln_guide_tree(self.h, n, _ptr(flat), stride, alnlen, gap[0], _ptr(tasks), _ptr(sd), _ptr(dm)))
    return (tasks, sd, dm) if want_dm else (tasks, sd)


Context.aln_guide_tree = _aln_guide_tree


def _three_encodings(tree_codes, codes, letters):
    """the sequences in the tree alphabet, in the alignment alphabet and as letters, flattened: (tflat, cflat, lflat, off, lens)"""
    tflat, off, lens = _flatten(tree_codes)
    cflat, _, _ = _flatten(codes)
    lflat = np.ascontiguousarray(np.concatenate([np.frombuffer(x.encode() if isinstance(x, str) else bytes(x), np.uint8) for x in letters]))
    if len(lflat) != len(cflat) or len(tflat) != len(cflat):
        raise KalignAmdError("the three encodings of the sequences differ in length")
    return tflat, cflat, lflat, off, lens


def _run_encoded(self, tree_codes, codes, letters, subm, scal, n_anchors=0, weight=2.0, realign=0, dm_scale=None,
                 n_threads=1, gap=b"-", refine=0):
    """ka_run_encoded(_refine): guide tree, (consistency,) alignment, `realign` realignment iterations, (refinement,)
    rows -- one call.  refine: 0, 1, 2 (| 256 adaptive budget) or 3, as kalign_run_seeded's argument.
    Returns the aligned rows (bytes) in the order of the input sequences."""
    tflat, cflat, lflat, off, lens = _three_encodings(tree_codes, codes, letters)
    n = len(codes)
    sub = np.ascontiguousarray(subm, np.float32).reshape(-1)
    sc = np.ascontiguousarray(scal, np.float32)
    dms = _dm_scale(dm_scale, n)
    alen = np.zeros(n, np.int32)
    args = (self.h, n, _ptr(tflat), _ptr(cflat), _ptr(lflat), _ptr(off), _ptr(lens), _ptr(sub), _ptr(sc),
            int(n_anchors), float(weight), int(realign), _ptr(dms), int(n_threads), gap[0])
    if refine:
        self._chk(self.L.ka_run_encoded_refine(*args[:14], int(refine), args[14], None, 0, _ptr(alen)))
    else:
        self._chk(self.L.ka_run_encoded(*args, None, 0, _ptr(alen)))        # the alignment stays in HBM: how long is it?
    self._job = dict(lens=lens, ntasks=n - 1, n=n)
    return self.tree_aligned_rows(letters, gap=gap)


Context.run_encoded = _run_encoded


def _fam_first(sizes):
    first = np.zeros(len(sizes) + 1, np.int32)
    first[1:] = np.cumsum(sizes)
    return first


def _dm_scale_forest(noise, sizes):
    if noise is None:
        return None
    noise = np.ascontiguousarray(np.concatenate([np.asarray(b, np.float32).reshape(-1) for b in noise]), np.float32)
    if len(noise) != sum(int(n) * min(32, int(n)) for n in sizes):
        raise KalignAmdError("dm_scale needs one block of n * min(32, n) multipliers per family")
    return noise


def _split_forest(tasks, sizes):
    """the forest task list (ka_guide_forest's numbering) as one array per family, still in the forest's numbering"""
    out, t = [], 0
    for n in sizes:
        out.append(tasks[t:t + int(n) - 1])
        t += int(n) - 1
    return out


def _guide_forest(self, families, n_threads=1, dm_scale=None):
    """ka_guide_forest: the guide trees of a batch of families with both distance batches on the device, two launches of
    ka_bpm_batch for all of them.  families: one list of sequences (tree alphabet) per family; dm_scale: None or one block
    of multipliers per family.  Returns (tasks[numseq - n_fam, 3] in the forest's numbering, seq_distances[numseq])."""
    sizes = [len(f) for f in families]
    flat, off, lens = _flatten([c for f in families for c in f])
    first = _fam_first(sizes)
    tasks = np.zeros((max(len(lens) - len(sizes), 0), 3), np.int32)
    sd = np.zeros(len(lens), np.float32)
    sc = _dm_scale_forest(dm_scale, sizes)
    nt = C.c_int(0)
    self._chk(self.L.ka_guide_forest(self.h, len(sizes), _ptr(first), _ptr(flat), _ptr(off), _ptr(lens), int(n_threads), _ptr(sc),
                                     _ptr(tasks) if len(tasks) else None, C.byref(nt), _ptr(sd)))
    return tasks[:nt.value], sd


Context.guide_forest = _guide_forest


def _aln_guide_forest(self, families=None, sizes=None, gap=b"-", want_dm=False):
    """ka_aln_guide_forest: the realignment trees of a batch of families.  families: per family a list of equal-length rows
    (bytes); or None with sizes = the number of sequences per family for the rows the last tree_aligned_rows left in HBM.
    Returns (tasks in the forest's numbering, seq_distances[, one n_f x n_f distance matrix per family])."""
    if families is None:
        sizes = [int(n) for n in sizes]
        flat, stride, widths = None, 0, None
    else:
        sizes = [len(f) for f in families]
        widths = np.array([len(f[0]) for f in families], np.int32)
        if any(len(r) != w for f, w in zip(families, widths) for r in f):
            raise KalignAmdError("rows of one alignment have one length")
        stride = int(widths.max())
        buf = np.full((sum(sizes), stride), gap[0], np.uint8)
        i = 0
        for f, w in zip(families, widths):
            for r in f:
                buf[i, :w] = np.frombuffer(bytes(r), np.uint8)
                i += 1
        flat = buf.reshape(-1)
    first = _fam_first(sizes)
    n = int(first[-1])
    tasks = np.zeros((max(n - len(sizes), 1), 3), np.int32)
    sd = np.zeros(n, np.float32)
    dm = np.zeros(sum(k * k for k in sizes), np.float32) if want_dm else None
    self._chk(self.L.ka_aln_guide_forest(self.h, len(sizes), _ptr(first), _ptr(flat), stride, _ptr(widths), gap[0], _ptr(tasks), _ptr(sd), _ptr(dm)))
    tasks = tasks[:n - len(sizes)]
    if not want_dm:
        return tasks, sd
    out, o = [], 0
    for k in sizes:
        out.append(dm[o:o + k * k].reshape(k, k))
        o += k * k
    return tasks, sd, out


Context.aln_guide_forest = _aln_guide_forest


def _run_families(self, families, subm, scal, n_anchors=0, weight=2.0, realign=0, refine=0, dm_scale=None, n_threads=4, gap=b"-"):
    """ka_run_encoded_batch: a batch of families from letters to rows in one call.  families: a list of
    (tree_codes, codes, letters), each as run_encoded takes them; all share subm / scal.  Every family is aligned as
    run_encoded aligns it alone; refine as run_encoded's (2, KALIGN_REFINE_CONFIDENT: the median of every family's own
    edges, batch_refine_stats says what it came to).  Returns one list of rows (bytes, in the order of the family's sequences) per family."""
    sizes = [len(f[1]) for f in families]
    if not sizes or min(sizes) < 1:
        raise KalignAmdError("run_families: every family needs a sequence")
    tree_codes = [x for f in families for x in f[0]]
    codes = [x for f in families for x in f[1]]
    letters = [x for f in families for x in f[2]]
    tflat, cflat, lflat, off, lens = _three_encodings(tree_codes, codes, letters)
    first = _fam_first(sizes)
    sub = np.ascontiguousarray(subm, np.float32).reshape(-1)
    sc = np.ascontiguousarray(scal, np.float32)
    dms = _dm_scale_forest(dm_scale, sizes)
    alen = np.zeros(len(lens), np.int32)
    self._chk(self.L.ka_run_encoded_batch(self.h, len(sizes), _ptr(first), _ptr(tflat), _ptr(cflat), _ptr(lflat), _ptr(off), _ptr(lens),
                                          _ptr(sub), _ptr(sc), int(n_anchors), float(weight), int(realign), _ptr(dms), int(n_threads),
                                          int(refine), gap[0], _ptr(alen)))
    return self.batch_rows(sizes, alen)


def _batch_rows(self, sizes, alen):
    """ka_batch_rows: the packed rows of the last run_families as one list of bytes per family"""
    need = int(self.L.ka_batch_rows_size(self.h))
    if need < 0:
        raise KalignAmdError("no finished batch on this context")
    buf = np.zeros(max(need, 1), np.uint8)
    self._chk(self.L.ka_batch_rows(self.h, _ptr(buf), need))
    out, o, i = [], 0, 0
    for n in sizes:
        w = int(alen[i])
        out.append([buf[o + k * (w + 1):o + k * (w + 1) + w].tobytes() for k in range(n)])
        o += n * (w + 1)
        i += n
    assert o == need
    return out


def _batch_stats(self):
    """ka_batch_stats of the last run_families: dict of device ms per stage, forest jobs run and wall ms"""
    out = np.zeros(6, np.float64)
    self._chk(self.L.ka_batch_stats(self.h, _ptr(out)))
    return dict(guide_dist_ms=out[0], dp_ms=out[1], realign_tree_ms=out[2], rows_ms=out[3], jobs=int(out[4]), wall_ms=out[5])


def _batch_refine_stats(self, n_fam):
    """ka_batch_refine_stats of the last run_families(refine=2): per family in input order, dict of thr (float32, the
    family's median confidence; 0 for a family of one sequence), edges (its tasks) and refined (those at or below thr)"""
    n_fam = int(n_fam)
    thr, edges, refined = np.zeros(max(n_fam, 1), np.float32), np.zeros(max(n_fam, 1), np.int32), np.zeros(max(n_fam, 1), np.int32)
    self._chk(self.L.ka_batch_refine_stats(self.h, n_fam, _ptr(thr), _ptr(edges), _ptr(refined)))
    return dict(thr=thr[:n_fam], edges=edges[:n_fam], refined=refined[:n_fam])


def refine_marks(numseq, tasks, conf, pooled=False):
    """ka_debug_refine_marks (no GPU, no context): the edges a mode-2 refinement pass marks -- tasks[n_tasks, 3] as
    tree_upload takes them, a confidence per task; pooled: tree_refine's one median over the job, else tree_refine_trees'
    median per tree.  Returns (tree_of[n_tasks], thr[n_trees], marks[n_tasks])."""
    L = load_library()
    tasks = np.ascontiguousarray(tasks, np.int32).reshape(-1, 3)
    cf = np.ascontiguousarray(conf, np.float32)
    nt = len(tasks)
    if len(cf) != nt:
        raise KalignAmdError("refine_marks: one confidence per task")
    tree_of, thr, marks, n = np.zeros(max(nt, 1), np.int32), np.zeros(max(nt, 1), np.float32), np.zeros(max(nt, 1), np.int32), C.c_int(0)
    if L.ka_debug_refine_marks(int(numseq), nt, _ptr(tasks), _ptr(cf), int(bool(pooled)), _ptr(tree_of), _ptr(thr), _ptr(marks), C.byref(n)):
        raise KalignAmdError(L.ka_last_error().decode())
    return tree_of[:nt], thr[:n.value].copy(), marks[:nt]


Context.run_families = _run_families
Context.batch_refine_stats = _batch_refine_stats
Context.batch_rows = _batch_rows
Context.batch_stats = _batch_stats


def residue_lens(rows):
    """letters per row (bytes / str, any lengths) as int32: a residue is an ASCII letter, every other byte a gap
    (ka_msa_is_residue, csrc/ka_msa.h)"""
    out = np.zeros(len(rows), np.int32)
    for k, r in enumerate(rows):
        b = np.frombuffer(r.encode() if isinstance(r, str) else bytes(r), np.uint8) | 32
        out[k] = np.count_nonzero((b >= 97) & (b <= 122))
    return out


class _CtxChild:
    """a handle that borrows its context's stream (Ensemble, Comparer): registered with the context, which closes it
    before it closes itself (Context.close); _destroy names the C function that frees the handle"""
    h = None

    def _adopt(self, ctx, h):
        self.h = h
        if not hasattr(ctx, "_children"):
            ctx._children = weakref.WeakSet()
        ctx._children.add(self)

    def close(self):
        """frees the device state; a closed context has closed its children already"""
        if self.h:
            getattr(self.L, self._destroy)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _rows_array(rows, n):
    """equal-length rows (bytes / str) -> (uint8[n, width], width)"""
    rows = [x.encode() if isinstance(x, str) else bytes(x) for x in rows]
    if len(rows) != n:
        raise KalignAmdError("%d rows for %d sequences" % (len(rows), n))
    width = len(rows[0]) if rows else 0
    if any(len(r) != width for r in rows):
        raise KalignAmdError("rows of one alignment have one length")
    return np.frombuffer(b"".join(rows), np.uint8).reshape(n, width), width


class Ensemble(_CtxChild):
    """The consensus stage of an ensemble (ka_ens): the members' rows on the device, then scores, the consensus alignment
    and confidences of any alignment of the same sequences.  Rows are in the members' sequence order.
    With table= (a POAR file's path, or its bytes) the support comes from that table instead of members
    (Context.ensemble_from_table): n_runs is the file's, add_member fails, everything else works the same."""
    _destroy = "ka_ens_destroy"

    def __init__(self, ctx, lens, n_runs=None, table=None):
        self.ctx, self.L = ctx, ctx.L
        self.lens = np.ascontiguousarray(lens, np.int32)
        self.n = len(self.lens)
        h = C.c_void_p()
        if not ctx.h:
            raise KalignAmdError("the context is closed")
        if table is None and n_runs is None:
            raise KalignAmdError("an Ensemble takes n_runs members or a POAR table")
        if table is None:
            ctx._chk(self.L.ka_ens_create(ctx.h, self.n, _ptr(self.lens), int(n_runs), C.byref(h)))
        elif isinstance(table, (bytes, bytearray, memoryview, np.ndarray)):
            img = np.frombuffer(bytes(table), np.uint8)
            ctx._chk(self.L.ka_ens_open_table_image(ctx.h, self.n, _ptr(self.lens), _ptr(img if len(img) else np.zeros(1, np.uint8)),
                                                    len(img), C.byref(h)))
        else:
            ctx._chk(self.L.ka_ens_open_table(ctx.h, self.n, _ptr(self.lens), os.fsencode(table), C.byref(h)))
        self._adopt(ctx, h)
        self.n_runs = int(self.L.ka_ens_n_runs(h))

    def add_member(self, k, rows):
        a, w = _rows_array(rows, self.n)
        self.ctx._chk(self.L.ka_ens_add_member(self.h, int(k), _ptr(a), w, w))

    def score(self, rows):
        """(sum of (support - 1) over the alignment's residue pairs, score_alignment_poar's value)"""
        a, w = _rows_array(rows, self.n)
        s, v = C.c_longlong(), C.c_double()
        self.ctx._chk(self.L.ka_ens_score_rows(self.h, _ptr(a), w, w, C.byref(s), C.byref(v)))
        return s.value, v.value

    def consensus(self, letters, min_support):
        """build_consensus at min_support: the consensus rows (bytes), letters = the sequences (str / bytes) placed in them"""
        flat = np.frombuffer(b"".join(x.encode() if isinstance(x, str) else bytes(x) for x in letters), np.uint8)
        if len(flat) != int(self.lens.sum()):
            raise KalignAmdError("letters do not match the sequence lengths")
        w = C.c_int()
        rc = self.L.ka_ens_consensus(self.h, int(min_support), _ptr(flat), None, 0, C.byref(w))
        if rc != ERR_ROWS_STRIDE:                                # asked for the width first
            self.ctx._chk(rc)
        out = np.zeros((self.n, max(w.value, 1)), np.uint8)
        self.ctx._chk(self.L.ka_ens_consensus(self.h, int(min_support), _ptr(flat), _ptr(out), out.shape[1], C.byref(w)))
        return [out[s, :w.value].tobytes() for s in range(self.n)]

    def confidence(self, rows):
        """compute_residue_confidence: (float32[n, width] per residue, 0 at gaps; float32[width] per column)"""
        a, w = _rows_array(rows, self.n)
        res = np.zeros((self.n, w), np.float32)
        col = np.zeros(w, np.float32)
        self.ctx._chk(self.L.ka_ens_confidence(self.h, _ptr(a), w, w, _ptr(res), _ptr(col)))
        return res, col

    def stats(self):
        """measurements of the last calls (ka_ens_stats) as a dict"""
        st = np.zeros(10, np.float64)
        cnt = np.zeros(33, np.int64)
        ms = np.zeros(33, np.float64)
        self.ctx._chk(self.L.ka_ens_stats(self.h, _ptr(st), _ptr(cnt), _ptr(ms)))
        keys = ["maps_ms", "score_ms", "count_ms", "write_ms", "greedy_host_ms", "columns_host_ms", "confidence_ms",
                "wait_host_ms", "chunks", "bfs_truncations"]
        out = dict(zip(keys, st.tolist()))
        out["level_candidates"] = {L: int(cnt[L]) for L in range(33) if cnt[L]}
        out["level_ms"] = {L: float(ms[L]) for L in range(33) if cnt[L] or ms[L]}
        tab = np.zeros(6, np.float64)
        self.ctx._chk(self.L.ka_ens_table_stats(self.h, _ptr(tab)))
        out.update(zip(["table_count_ms", "table_write_ms", "table_host_ms", "table_entries", "table_chunks", "table_wait_host_ms"],
                       tab.tolist()))
        return out

    # ---- the POAR table as a file (poar_table_write / poar_table_read, lib/src/poar.c:203-325) ----
    def table_size(self):
        """(bytes of the POAR file, its entries)"""
        b, n = C.c_longlong(), C.c_longlong()
        self.ctx._chk(self.L.ka_ens_table_size(self.h, C.byref(b), C.byref(n)))
        return b.value, n.value

    def write_table(self, path):
        """the file poar_table_write writes for these members (kalign_ensemble's save_poar_path), byte for byte"""
        self.ctx._chk(self.L.ka_ens_table_write(self.h, os.fsencode(path)))

    def table_image(self):
        """the same bytes in memory"""
        out = np.zeros(self.table_size()[0], np.uint8)
        self.ctx._chk(self.L.ka_ens_table_image(self.h, _ptr(out), len(out)))
        return out.tobytes()

    # ---- new tables from tables (ka_ens_merge / ka_ens_select): the operands stay as they are, the result is a new Ensemble ----
    def _derived(self, h):
        e = object.__new__(Ensemble)
        e.ctx, e.L, e.lens, e.n = self.ctx, self.L, self.lens, self.n
        e._adopt(self.ctx, h)
        e.n_runs = int(self.L.ka_ens_n_runs(h))
        return e

    def merge(self, other):
        """a table-backed Ensemble of this one's members followed by other's (member k of other becomes n_runs + k): the
        union of the two POAR tables.  Both hold the same sequences in one context, every member added or opened from a table."""
        if not isinstance(other, Ensemble):
            raise KalignAmdError("merge takes another Ensemble")
        h = C.c_void_p()
        self.ctx._chk(self.L.ka_ens_merge(self.h, other.h, C.byref(h)))
        return self._derived(h)

    def select(self, members):
        """a table-backed Ensemble of members[0], members[1], ... of this one, in that order (distinct indices); the
        entries of the table that none of them holds are dropped"""
        m = np.ascontiguousarray(list(members), np.int32)
        h = C.c_void_p()
        self.ctx._chk(self.L.ka_ens_select(self.h, _ptr(m if len(m) else np.zeros(1, np.int32)), len(m), C.byref(h)))
        return self._derived(h)


def _ens_create(self, lens, n_runs):
    """ka_ens_create: an Ensemble for sequences of these lengths and n_runs members"""
    return Ensemble(self, lens, n_runs)


Context.ensemble = _ens_create


def _ens_from_table(self, lens, path=None, image=None):
    """ka_ens_open_table: an Ensemble whose support comes from a POAR file (path) or its bytes (image)"""
    if (path is None) == (image is None):
        raise KalignAmdError("ensemble_from_table takes a path or an image")
    return Ensemble(self, lens, table=path if image is None else bytes(image))


Context.ensemble_from_table = _ens_from_table


def check_table(image_or_path, lens):
    """ka_poar_check_image: the reader's checks of a POAR file (its bytes, or its path) against sequences of these lengths,
    on the host alone; returns (n_runs, entries) or raises with the cause"""
    L = load_library()
    if isinstance(image_or_path, (bytes, bytearray, memoryview, np.ndarray)):
        data = bytes(image_or_path)
    else:
        with open(image_or_path, "rb") as f:
            data = f.read()
    img = np.frombuffer(data, np.uint8)
    lens = np.ascontiguousarray(lens, np.int32)
    r, n = C.c_int(), C.c_longlong()
    if L.ka_poar_check_image(_ptr(img if len(img) else np.zeros(1, np.uint8)), len(img), len(lens), _ptr(lens), C.byref(r), C.byref(n)):
        raise KalignAmdError(L.ka_last_error().decode())
    return r.value, n.value


CMP_COUNTS = ["ref_total_aligned_pairs", "ref_total_gap_pairs", "identical_aligned", "identical_gaps",
              "test_total_aligned_pairs", "test_total_gap_pairs", "ref_scored_pairs", "test_pairs", "common_scored",
              "common_all", "tc_correct", "tc_total"]


def _cmp_result(counts, scores, sp):
    """one test's outputs of ka_cmp_score as a dict: python-kalign's keys (compare, compare_detailed), then the raw counts"""
    d = dict(sp=float(sp), recall=float(scores[0]), precision=float(scores[1]), f1=float(scores[2]), tc=float(scores[3]),
             ref_pairs=int(counts[6]), test_pairs=int(counts[7]), common_pairs=int(counts[8]), sp_double=float(scores[4]))
    d.update({k: int(v) for k, v in zip(CMP_COUNTS, counts)})
    return d


CMP_DETAIL_STATS = ["maps_ms", "walk_ms", "columns_ms", "launches", "syncs"]


def _detail_buffers(T, n_tcols, n_rcols):
    """the seven outputs of ka_cmp_detail / ka_cmp_fam_detail, in the order the entries take them"""
    return [np.zeros((3, T), np.int32), np.zeros(n_tcols, np.int32), np.zeros(n_tcols, np.int64), np.zeros(n_tcols, np.uint8),
            np.zeros(n_rcols, np.int32), np.zeros(n_rcols, np.int64), np.zeros(n_rcols, np.uint8)]


def _detail_result(bufs, res_first, tcol_first, rcol_first):
    """the outputs split per family: res [n_residues, 3] (aligned partners in the reference, in the test, in both), and
    test_columns / ref_columns as dicts of residues (k), common and correct"""
    planes, tk, tc, tf, rk, rc, rf = bufs
    out = []
    for f in range(len(res_first) - 1):
        t0, t1, r0, r1 = tcol_first[f], tcol_first[f + 1], rcol_first[f], rcol_first[f + 1]
        out.append(dict(res=np.ascontiguousarray(planes[:, res_first[f]:res_first[f + 1]].T),
                        test_columns=dict(residues=tk[t0:t1].copy(), common=tc[t0:t1].copy(), correct=tf[t0:t1].copy()),
                        ref_columns=dict(residues=rk[r0:r1].copy(), common=rc[r0:r1].copy(), correct=rf[r0:r1].copy())))
    return out


def _detail_stats(L, fn, ctx, h):
    st = np.zeros(5, np.float64)
    ctx._chk(getattr(L, fn)(h, _ptr(st)))
    d = dict(zip(CMP_DETAIL_STATS, st.tolist()))
    d["launches"], d["syncs"] = int(d["launches"]), int(d["syncs"])
    return d


class Comparer(_CtxChild):
    """A reference alignment on the device (ka_cmp) that test alignments of the same sequences are scored against, as
    kalign_msa_compare (sp) and kalign_msa_compare_detailed / _with_mask (recall, precision, f1, tc) score them.  Rows
    are paired by position: kalign_amd.compare pairs named rows the way the reference does."""
    _destroy = "ka_cmp_destroy"

    def __init__(self, ctx, ref_rows):
        self.ctx, self.L = ctx, ctx.L
        if not ctx.h:
            raise KalignAmdError("the context is closed")
        rows = list(ref_rows)
        self.n = len(rows)
        if self.n < 2:
            raise KalignAmdError("a comparison needs two sequences at least (%d given)" % self.n)
        a, w = _rows_array(rows, self.n)
        self.width = w
        self.lens = residue_lens(rows)
        h = C.c_void_p()
        ctx._chk(self.L.ka_cmp_create(ctx.h, self.n, _ptr(self.lens), _ptr(a), w, w, C.byref(h)))
        self._adopt(ctx, h)

    def _set_mask(self, max_gap_frac, column_mask):
        if column_mask is None:
            self.ctx._chk(self.L.ka_cmp_set_mask(self.h, float(max_gap_frac), None, 0))
        else:
            m = np.ascontiguousarray(column_mask, np.int32).reshape(-1)
            self.ctx._chk(self.L.ka_cmp_set_mask(self.h, float(max_gap_frac), _ptr(m), len(m)))

    def _test_array(self, rows):
        rows = list(rows)
        if len(rows) != self.n:
            raise KalignAmdError("the test alignment has %d rows, the reference %d" % (len(rows), self.n))
        return _rows_array(rows, self.n)

    def score(self, test_rows, max_gap_frac=-1.0, column_mask=None):
        """one test alignment: column_mask (one int per reference column, non-zero = scored) as
        kalign_msa_compare_with_mask, else max_gap_frac as kalign_msa_compare_detailed (< 0: every column)"""
        return self.score_many([test_rows], max_gap_frac, column_mask)[0]

    def score_many(self, tests, max_gap_frac=-1.0, column_mask=None):
        """several test alignments of the same sequences against the reference (ka_cmp_score_batch): what score()
        returns for each"""
        if not self.h:
            raise KalignAmdError("the comparer is closed")
        self._set_mask(max_gap_frac, column_mask)
        arrs = [self._test_array(t) for t in tests]
        K = len(arrs)
        if K == 0:
            return []
        ptrs = (C.c_void_p * K)(*[a.ctypes.data for a, _ in arrs])
        strides = np.array([w for _, w in arrs], np.int64)
        widths = np.array([w for _, w in arrs], np.int32)
        counts = np.zeros((K, 12), np.int64)
        scores = np.zeros((K, 5), np.float64)
        sp = np.zeros(K, np.float32)
        self.ctx._chk(self.L.ka_cmp_score_batch(self.h, K, ptrs, _ptr(strides), _ptr(widths), _ptr(counts), _ptr(scores), _ptr(sp)))
        return [_cmp_result(counts[k], scores[k], sp[k]) for k in range(K)]

    def stats(self):
        """device ms (ka_cmp_stats): the reference's maps, then the test maps, the walk and TC of the last score call"""
        st = np.zeros(4, np.float64)
        self.ctx._chk(self.L.ka_cmp_stats(self.h, _ptr(st)))
        return dict(zip(["ref_maps_ms", "maps_ms", "walk_ms", "tc_ms"], st.tolist()))

    def detail(self, test_rows):
        """where the test alignment agrees with the reference (ka_cmp_detail): dict(res=[n_residues, 3] int32 -- a
        residue's aligned partners in the reference, in the test and in both, residues numbered sequence by sequence --,
        test_columns, ref_columns = dicts of residues (k), common and correct per column).  test_columns["correct"] is
        _column_correctness of the reference's calibration benchmark; the column rule of score() plays no part."""
        if not self.h:
            raise KalignAmdError("the comparer is closed")
        a, w = self._test_array(test_rows)
        T = int(self.lens.sum())
        bufs = _detail_buffers(T, w, self.width)
        self.ctx._chk(self.L.ka_cmp_detail(self.h, _ptr(a), w, w, *[_ptr(b) for b in bufs]))
        return _detail_result(bufs, [0, T], [0, w], [0, self.width])[0]

    def detail_stats(self):
        """ka_cmp_detail_stats: device ms of the test maps, the detailed walk and the column pass, then the launches and
        host synchronisations of the last detail() call"""
        return _detail_stats(self.L, "ka_cmp_detail_stats", self.ctx, self.h)


def _cmp_create(self, ref_rows):
    """ka_cmp_create: a Comparer holding ref_rows (one row per sequence) on this context's device"""
    return Comparer(self, ref_rows)


Context.comparer = _cmp_create


def pack_families(families):
    """lists of equal-length rows (bytes / str), one list per family -> (uint8 rows packed as ka_batch_rows packs them: the
    rows of family f alnlen_f + 1 bytes apart, a 0 byte after each; int32 alnlen per family)"""
    fams = [[x.encode() if isinstance(x, str) else bytes(x) for x in f] for f in families]
    widths = np.array([len(f[0]) if f else 0 for f in fams], np.int32)
    for k, (f, w) in enumerate(zip(fams, widths)):
        if any(len(r) != w for r in f):
            raise KalignAmdError("family %d: rows of one alignment have one length" % k)
    packed = np.frombuffer(b"".join(r + b"\0" for f in fams for r in f), np.uint8)
    return packed, widths


class FamilyComparer(_CtxChild):
    """The reference alignments of a batch of families on the device (ka_cmp_fam): score() takes one test alignment per
    family and returns, per family, what Comparer(ref).score(test) returns for it alone -- in a number of launches that
    does not grow with the batch.  refs / tests: one list of rows per family (what Context.run_families returns), rows
    paired by position: kalign_amd.compare.compare_families pairs named rows."""
    _destroy = "ka_cmp_fam_destroy"

    def __init__(self, ctx, refs):
        self.ctx, self.L = ctx, ctx.L
        if not ctx.h:
            raise KalignAmdError("the context is closed")
        refs = [list(f) for f in refs]
        if not refs:
            raise KalignAmdError("a family comparison needs a family")
        self.sizes = [len(f) for f in refs]
        self.first = _fam_first(self.sizes)
        self.lens = residue_lens([r for f in refs for r in f])
        rows, self.widths = pack_families(refs)
        h = C.c_void_p()
        ctx._chk(self.L.ka_cmp_fam_create(ctx.h, len(refs), _ptr(self.first), _ptr(self.lens), _ptr(rows if len(rows) else np.zeros(1, np.uint8)),
                                          _ptr(self.widths), C.byref(h)))
        self._adopt(ctx, h)

    def _set_masks(self, max_gap_frac, column_masks):
        F = len(self.sizes)
        frac = np.ascontiguousarray(np.broadcast_to(np.asarray(max_gap_frac, np.float32), (F,)))
        masks, off = pack_masks(column_masks, self.widths, "reference alignment")
        self.ctx._chk(self.L.ka_cmp_fam_set_masks(self.h, _ptr(frac), _ptr(masks), _ptr(off)))

    def score(self, tests, max_gap_frac=-1.0, column_masks=None):
        """one test alignment per family.  max_gap_frac: one value or one per family (kalign_msa_compare_detailed; < 0:
        every column); column_masks: None, or per family None or one int per reference column
        (kalign_msa_compare_with_mask).  Returns one Comparer.score dict per family."""
        if not self.h:
            raise KalignAmdError("the comparer is closed")
        tests = self._tests(tests)
        self._set_masks(max_gap_frac, column_masks)
        rows, widths = pack_families(tests)
        F = len(self.sizes)
        counts = np.zeros((F, 12), np.int64)
        scores = np.zeros((F, 5), np.float64)
        sp = np.zeros(F, np.float32)
        self.ctx._chk(self.L.ka_cmp_fam_score(self.h, _ptr(rows if len(rows) else np.zeros(1, np.uint8)), _ptr(widths), _ptr(counts), _ptr(scores), _ptr(sp)))
        return [_cmp_result(counts[f], scores[f], sp[f]) for f in range(F)]

    def stats(self):
        """device ms (ka_cmp_fam_stats): the references' maps, then the test maps, the walk and TC of the last score call"""
        st = np.zeros(4, np.float64)
        self.ctx._chk(self.L.ka_cmp_fam_stats(self.h, _ptr(st)))
        return dict(zip(["ref_maps_ms", "maps_ms", "walk_ms", "tc_ms"], st.tolist()))

    def _tests(self, tests):
        tests = [list(f) for f in tests]
        if [len(f) for f in tests] != self.sizes:
            for f, (t, n) in enumerate(zip(tests, self.sizes)):
                if len(t) != n:
                    raise KalignAmdError("family %d: the test alignment has %d rows, the reference %d" % (f, len(t), n))
            raise KalignAmdError("%d test alignments for %d families" % (len(tests), len(self.sizes)))
        return tests

    def detail(self, tests, want=None):
        """one test alignment per family (ka_cmp_fam_detail): per family what Comparer(ref).detail(test) returns for it
        alone, from launches that do not grow with the batch.  want: None, or the outputs asked of the device, a subset of
        range(7) in the entry's order (the others stay zero) -- for the tests of the optional pointers."""
        if not self.h:
            raise KalignAmdError("the comparer is closed")
        rows, widths = pack_families(self._tests(tests))
        seq_first = np.asarray(self.first, np.int64)
        res_first = np.concatenate([[0], np.cumsum(self.lens, dtype=np.int64)])[seq_first]
        tcol_first = np.concatenate([[0], np.cumsum(widths, dtype=np.int64)])
        rcol_first = np.concatenate([[0], np.cumsum(self.widths, dtype=np.int64)])
        bufs = _detail_buffers(int(res_first[-1]), int(tcol_first[-1]), int(rcol_first[-1]))
        ptrs = [_ptr(b) if want is None or k in want else None for k, b in enumerate(bufs)]
        self.ctx._chk(self.L.ka_cmp_fam_detail(self.h, _ptr(rows if len(rows) else np.zeros(1, np.uint8)), _ptr(widths), *ptrs))
        return _detail_result(bufs, res_first, tcol_first, rcol_first)

    def detail_stats(self):
        """ka_cmp_fam_detail_stats: as Comparer.detail_stats, over the whole batch"""
        return _detail_stats(self.L, "ka_cmp_fam_detail_stats", self.ctx, self.h)


def _cmp_fam_create(self, refs):
    """ka_cmp_fam_create: a FamilyComparer holding one reference alignment per family on this context's device"""
    return FamilyComparer(self, refs)


Context.family_comparer = _cmp_fam_create


ENS_FAM_STATS = ["maps_ms", "score_ms", "count_ms", "write_ms", "confidence_ms", "greedy_threads_host_ms", "greedy_wall_host_ms",
                 "wait_host_ms", "chunks", "candidates", "bfs_truncations", "add_member_launches", "add_member_syncs",
                 "score_members_launches", "score_members_syncs", "score_launches", "score_syncs", "consensus_launches",
                 "consensus_syncs", "confidence_launches", "confidence_syncs"]


def _unpack_families(buf, sizes, widths):
    """packed rows (pack_families' layout) -> one list of bytes per family"""
    out, o = [], 0
    for n, w in zip(sizes, widths):
        w = int(w)
        out.append([buf[o + k * (w + 1):o + k * (w + 1) + w].tobytes() for k in range(n)])
        o += n * (w + 1)
    return out


class FamilyEnsemble(_CtxChild):
    """The consensus stage of the ensembles of a batch of families with the same number of members (ka_ens_fam): per family
    what an Ensemble of that family alone returns, in a number of launches and synchronisations that does not grow with
    the batch.  families_rows: one list of rows per family (what Context.run_families returns is a member as it stands).
    The POAR table as a file stays with Ensemble."""
    _destroy = "ka_ens_fam_destroy"

    def __init__(self, ctx, fam_lens, n_runs):
        self.ctx, self.L = ctx, ctx.L
        if not ctx.h:
            raise KalignAmdError("the context is closed")
        fam_lens = [np.ascontiguousarray(l, np.int32).reshape(-1) for l in fam_lens]
        if not fam_lens:
            raise KalignAmdError("a family ensemble needs a family")
        self.sizes = [len(l) for l in fam_lens]
        self.first = _fam_first(self.sizes)
        self.lens = np.ascontiguousarray(np.concatenate(fam_lens), np.int32)
        self.n_runs = int(n_runs)
        h = C.c_void_p()
        ctx._chk(self.L.ka_ens_fam_create(ctx.h, len(self.sizes), _ptr(self.first), _ptr(self.lens), self.n_runs, C.byref(h)))
        self._adopt(ctx, h)

    def _pack(self, families_rows, skip=False):
        if not self.h:
            raise KalignAmdError("the family ensemble is closed")
        fams = [None if f is None else list(f) for f in families_rows]
        if len(fams) != len(self.sizes):
            raise KalignAmdError("%d alignments for %d families" % (len(fams), len(self.sizes)))
        for f, (t, n) in enumerate(zip(fams, self.sizes)):
            if t is None:
                if not skip:
                    raise KalignAmdError("family %d: no rows" % f)
            elif len(t) != n:
                raise KalignAmdError("family %d: the alignment has %d rows, the family %d sequences" % (f, len(t), n))
        rows, widths = pack_families([t for t in fams if t is not None])
        w = np.full(len(fams), -1, np.int32)
        w[[f for f, t in enumerate(fams) if t is not None]] = widths
        return (rows if len(rows) else np.zeros(1, np.uint8)), w

    def add_member(self, k, families_rows):
        rows, w = self._pack(families_rows)
        self.ctx._chk(self.L.ka_ens_fam_add_member(self.h, int(k), _ptr(rows), _ptr(w)))

    def score_members(self):
        """(sums int64[n_runs, families], scores float64[n_runs, families]): Ensemble.score of every member, from the maps
        on the device"""
        F = len(self.sizes)
        s = np.zeros((self.n_runs, F), np.int64)
        v = np.zeros((self.n_runs, F), np.float64)
        self.ctx._chk(self.L.ka_ens_fam_score_members(self.h, _ptr(s), _ptr(v)))
        return s, v

    def score(self, families_rows):
        """(sums int64[families], scores float64[families]); a None entry skips that family: its outputs are 0"""
        rows, w = self._pack(families_rows, skip=True)
        s = np.zeros(len(self.sizes), np.int64)
        v = np.zeros(len(self.sizes), np.float64)
        self.ctx._chk(self.L.ka_ens_fam_score(self.h, _ptr(rows), _ptr(w), _ptr(s), _ptr(v)))
        return s, v

    def consensus(self, families_letters, min_support, n_threads=4):
        """build_consensus per family at min_support (an int, or one per family): one list of consensus rows per family;
        families_letters: per family its sequences (str / bytes)"""
        if not self.h:
            raise KalignAmdError("the family ensemble is closed")
        flat = np.frombuffer(b"".join(x.encode() if isinstance(x, str) else bytes(x) for f in families_letters for x in f), np.uint8)
        if [len(f) for f in families_letters] != self.sizes or len(flat) != int(self.lens.sum()):
            raise KalignAmdError("letters do not match the families' sequence lengths")
        ms = np.ascontiguousarray(np.broadcast_to(np.asarray(min_support, np.int32), (len(self.sizes),)))
        w = np.zeros(len(self.sizes), np.int32)
        self.ctx._chk(self.L.ka_ens_fam_consensus(self.h, _ptr(ms), _ptr(flat if len(flat) else np.zeros(1, np.uint8)), int(n_threads), _ptr(w)))
        need = int(self.L.ka_ens_fam_rows_size(self.h))
        buf = np.zeros(max(need, 1), np.uint8)
        self.ctx._chk(self.L.ka_ens_fam_rows(self.h, _ptr(buf), need))
        return _unpack_families(buf, self.sizes, w)

    def confidence(self, families_rows):
        """per family (float32[n, width] per residue, 0 at gaps; float32[width] per column), as Ensemble.confidence"""
        rows, w = self._pack(families_rows)
        n = np.asarray(self.sizes, np.int64)
        res = np.zeros(max(int((n * w).sum()), 1), np.float32)
        col = np.zeros(max(int(w.sum()), 1), np.float32)
        self.ctx._chk(self.L.ka_ens_fam_confidence(self.h, _ptr(rows), _ptr(w), _ptr(res), _ptr(col)))
        out, o, c = [], 0, 0
        for k, x in zip(self.sizes, w):
            x = int(x)
            out.append((res[o:o + k * x].reshape(k, x).copy(), col[c:c + x].copy()))
            o += k * x
            c += x
        return out

    def stats(self):
        """measurements of the last calls (ka_ens_fam_stats) as a dict; the counts as ints"""
        st = np.zeros(len(ENS_FAM_STATS), np.float64)
        self.ctx._chk(self.L.ka_ens_fam_stats(self.h, _ptr(st)))
        return {k: (float(v) if k.endswith("_ms") else int(v)) for k, v in zip(ENS_FAM_STATS, st)}


def _ens_fam_create(self, fam_lens, n_runs):
    """ka_ens_fam_create: a FamilyEnsemble for families of sequences of these lengths (one list per family), n_runs members each"""
    return FamilyEnsemble(self, fam_lens, n_runs)


Context.family_ensemble = _ens_fam_create


SUM_COUNTS = ["gaps", "cells", "conserved_columns", "columns", "matching_pairs", "compared_pairs"]
SUM_STATS = ["table_ms", "consensus_ms", "keep_ms", "compact_ms", "launches", "syncs"]
IDENTITY_STATS = ["identity_ms", "launches", "syncs"]
GAP_COUNTS = ["n_seqs", "alignment_length", "characters", "total_gaps", "n_gap_blocks", "terminal_gaps", "internal_gaps", "n_gappy_columns"]
GAP_VALUES = ["mean_seq_length", "expansion_factor", "gap_fraction", "mean_gap_block_len", "mean_terminal_gap", "mean_internal_gap",
              "gappy_column_fraction"]
GAP_STATS = ["gaps_ms", "ungap_ms", "gaps_launches", "gaps_syncs", "ungap_launches", "ungap_syncs"]


def identity_entries(sizes):
    """ka_sum_fam_identity_entries: the entries of each identity matrix of a batch of families of these sizes, the sum of
    n * n -- on the host alone; raises where the batch is refused (an empty family, 2^31 entries or more)"""
    L = load_library()
    sizes = [int(n) for n in sizes]
    if any(n < 0 or n > 2 ** 31 - 1 for n in sizes) or sum(sizes) > 2 ** 31 - 1:
        raise KalignAmdError("family sizes are counts of rows, fewer than 2^31 in all")
    n = int(L.ka_sum_fam_identity_entries(len(sizes), _ptr(_fam_first(sizes))))
    if n < 0:
        raise KalignAmdError(L.ka_last_error().decode())
    return n


def pack_masks(column_masks, widths, what="alignment"):
    """per family None or a mask of its width -> (int32 masks back to back or None, int64 offsets, -1 where there is none):
    what ka_sum_fam_keep and ka_cmp_fam_set_masks take (FamilySummary, FamilyComparer: the one statement of the layout)"""
    F = len(widths)
    if column_masks is None:
        return None, None
    if len(column_masks) != F:
        raise KalignAmdError("%d column masks for %d families" % (len(column_masks), F))
    off, parts, o = np.full(F, -1, np.int64), [], 0
    for f, m in enumerate(column_masks):
        if m is None:
            continue
        m = np.ascontiguousarray(m, np.int32).reshape(-1)
        if len(m) != widths[f]:
            raise KalignAmdError("family %d: mask length %d != %s length %d" % (f, len(m), what, widths[f]))
        off[f] = o
        parts.append(m)
        o += len(m)
    return (np.concatenate(parts) if parts else None), off


class FamilySummary(_CtxChild):
    """The finished rows of a batch of families on the device (ka_sum_fam) and what python-kalign's kalign.utils computes
    from each -- column table, alignment_stats, consensus_sequence, the columns remove_gap_columns / trim_alignment keep,
    the trimmed rows -- bit for bit, in a number of launches that does not grow with the batch.  families_rows: one list
    of rows per family (what Context.run_families returns).  gap: the gap byte; every other byte is a character."""
    _destroy = "ka_sum_fam_destroy"

    def __init__(self, ctx, families_rows, gap=b"-"):
        self.ctx, self.L = ctx, ctx.L
        if not ctx.h:
            raise KalignAmdError("the context is closed")
        # (a str row is its latin-1 bytes, one byte per character, as kalign_amd.summary hands rows over)
        fams = [[x.encode("latin-1") if isinstance(x, str) else bytes(x) for x in f] for f in families_rows]
        if not fams:
            raise KalignAmdError("a family summary needs a family")
        gap = gap.encode() if isinstance(gap, str) else bytes(gap)
        if len(gap) != 1:
            raise KalignAmdError("the gap is one byte")
        self.gap = gap
        self.sizes = [len(f) for f in fams]
        self.first = _fam_first(self.sizes)
        rows, self.widths = pack_families(fams)
        self.col_first = np.concatenate([[0], np.cumsum(self.widths, dtype=np.int64)])
        h = C.c_void_p()
        ctx._chk(self.L.ka_sum_fam_create(ctx.h, len(fams), _ptr(self.first), _ptr(rows if len(rows) else np.zeros(1, np.uint8)),
                                          _ptr(self.widths), gap[0], C.byref(h)))
        self._adopt(ctx, h)

    def _open(self):
        if not self.h:
            raise KalignAmdError("the summary is closed")
        return len(self.sizes)

    def _split(self, a):
        return [a[self.col_first[f]:self.col_first[f + 1]] for f in range(len(self.sizes))]

    def _thresholds(self, t):
        return np.ascontiguousarray(np.broadcast_to(np.asarray(t, np.float64), (len(self.sizes),)))

    def columns(self):
        """per family a dict of per-column arrays: n_gap, n_distinct, top_char (uint8), top_count, same_pairs (int64)"""
        self._open()
        n = int(self.col_first[-1])
        g, d, tc, sp = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int64)
        ch = np.zeros(n, np.uint8)
        self.ctx._chk(self.L.ka_sum_fam_columns(self.h, _ptr(g), _ptr(d), _ptr(ch), _ptr(tc), _ptr(sp)))
        return [dict(n_gap=a, n_distinct=b, top_char=c, top_count=e, same_pairs=s)
                for a, b, c, e, s in zip(self._split(g), self._split(d), self._split(ch), self._split(tc), self._split(sp))]

    def summary(self):
        """per family alignment_stats' dict (length, n_sequences, gap_fraction, conservation, identity) and the six exact
        counts behind the three values (SUM_COUNTS)"""
        F = self._open()
        counts, values = np.zeros((F, 6), np.int64), np.zeros((F, 3), np.float64)
        self.ctx._chk(self.L.ka_sum_fam_summary(self.h, _ptr(counts), _ptr(values)))
        out = []
        for f in range(F):
            d = dict(length=int(self.widths[f]), n_sequences=self.sizes[f], gap_fraction=float(values[f, 0]),
                     conservation=float(values[f, 1]), identity=float(values[f, 2]))
            d.update({k: int(v) for k, v in zip(SUM_COUNTS, counts[f])})
            out.append(d)
        return out

    def consensus(self, threshold=0.5, want_ambiguous=False):
        """consensus_sequence of every family as bytes; threshold one value or one per family.  want_ambiguous: also the
        families' ambiguous characters (b"N" / b"X")"""
        F = self._open()
        out = np.zeros(int(self.col_first[-1]) + F, np.uint8)
        amb = np.zeros(F, np.uint8)
        self.ctx._chk(self.L.ka_sum_fam_consensus(self.h, _ptr(self._thresholds(threshold)), _ptr(out), _ptr(amb)))
        rows = [out[int(self.col_first[f]) + f:int(self.col_first[f + 1]) + f].tobytes() for f in range(F)]
        return (rows, [bytes([a]) for a in amb]) if want_ambiguous else rows

    def keep(self, gap_threshold=1.0, column_masks=None):
        """per family the int32 0 / 1 flags of its columns: a family's column mask (non-zero keeps) where column_masks
        gives one, else n_gap / n < gap_threshold (one value or one per family).  The list is column_masks of
        FamilyComparer.score / compare.compare_families as it stands."""
        self._open()
        masks, off = pack_masks(column_masks, self.widths)
        keep = np.zeros(int(self.col_first[-1]), np.int32)
        self.ctx._chk(self.L.ka_sum_fam_keep(self.h, _ptr(self._thresholds(gap_threshold)), _ptr(masks), _ptr(off), _ptr(keep), None))
        return self._split(keep)

    def compact(self, gap_threshold=1.0, column_masks=None):
        """the rows of every family with only the columns keep() keeps: one list of bytes per family"""
        F = self._open()
        masks, off = pack_masks(column_masks, self.widths)
        widths = np.zeros(F, np.int32)
        self.ctx._chk(self.L.ka_sum_fam_compact(self.h, _ptr(self._thresholds(gap_threshold)), _ptr(masks), _ptr(off), _ptr(widths)))
        n = int(self.L.ka_sum_fam_rows_size(self.h))
        buf = np.zeros(max(n, 1), np.uint8)
        self.ctx._chk(self.L.ka_sum_fam_rows(self.h, _ptr(buf), n))
        return _unpack_families(buf, self.sizes, widths)

    def stats(self):
        """ka_sum_fam_stats: device ms of the column table and of the last consensus, keep and compact; kernel launches and
        host synchronisations of the last of those calls (columns(), summary() and the hand-out of rows do not count)"""
        st = np.zeros(len(SUM_STATS), np.float64)
        self.ctx._chk(self.L.ka_sum_fam_stats(self.h, _ptr(st)))
        return {k: (float(v) if k.endswith("_ms") else int(v)) for k, v in zip(SUM_STATS, st)}


    def identity(self, want_counts=False):
        """pairwise_identity_matrix of every family: a float64 [n, n] array each -- matches / compared over the columns
        where both rows hold a character, 0.0 where there is none, 1.0 on the diagonal.  want_counts: per family
        (identity, matches, compared), the counts int32 [n, n].  The first call computes the matrices of the whole batch
        in one launch and leaves them on the device; later calls copy."""
        self._open()
        sq = np.array(self.sizes, np.int64) ** 2
        if int(sq.sum()) > 2 ** 31 - 1:
            total = 1                                             # (refused by the call below, which says why)
        else:
            total = int(sq.sum())
        ident = np.zeros(total, np.float64)
        m = np.zeros(total, np.int32) if want_counts else None
        c = np.zeros(total, np.int32) if want_counts else None
        self.ctx._chk(self.L.ka_sum_fam_identity(self.h, _ptr(m), _ptr(c), _ptr(ident)))
        first = np.concatenate([[0], np.cumsum(sq)])

        def blocks(a):
            return [a[first[f]:first[f + 1]].reshape(n, n) for f, n in enumerate(self.sizes)]

        return list(zip(blocks(ident), blocks(m), blocks(c))) if want_counts else blocks(ident)

    def identity_stats(self):
        """ka_sum_fam_identity_stats: device ms of the identity pass, kernel launches and host synchronisations of the
        identity() call that computed the matrices (zeros before it; unchanged by the calls that only copy)"""
        self._open()
        st = np.zeros(len(IDENTITY_STATS), np.float64)
        self.ctx._chk(self.L.ka_sum_fam_identity_stats(self.h, _ptr(st)))
        return {k: (float(v) if k.endswith("_ms") else int(v)) for k, v in zip(IDENTITY_STATS, st)}

    def gaps(self, want_rows=False):
        """the gap structure of every family, one dict each with GapStats' names (benchmarks/analysis.py:
        compute_gap_stats) -- n_seqs, alignment_length, mean_seq_length, expansion_factor, total_gaps, gap_fraction,
        n_gap_blocks, mean_gap_block_len, mean_terminal_gap, mean_internal_gap, n_gappy_columns, gappy_column_fraction --
        and gap_opens_per_seq (blocks / n), characters, terminal_gaps and internal_gaps (the sums behind the two means).
        want_rows: also rows, int32 [n, 4]: a row's characters, leading and trailing gap columns and gap blocks (an
        all-gap row: leading = trailing = width, one block).  The first call walks the rows of the whole batch on the
        device; later calls copy."""
        F = self._open()
        counts, values = np.zeros((F, len(GAP_COUNTS)), np.int64), np.zeros((F, len(GAP_VALUES)), np.float64)
        recs = np.zeros((int(self.first[-1]), 4), np.int32) if want_rows else None
        self.ctx._chk(self.L.ka_sum_fam_gaps(self.h, _ptr(counts), _ptr(values), _ptr(recs)))
        out = []
        for f in range(F):
            d = {k: int(v) for k, v in zip(GAP_COUNTS, counts[f])}
            d.update({k: float(v) for k, v in zip(GAP_VALUES, values[f])})
            d["gap_opens_per_seq"] = float(d["n_gap_blocks"]) / float(d["n_seqs"])
            if want_rows:
                d["rows"] = recs[self.first[f]:self.first[f + 1]]
            out.append(d)
        return out

    def ungapped(self, want_offsets=False):
        """the rows of every family without their gaps (dealign_msa): one list of bytes per family.  want_offsets: also
        the int64 [rows + 1] offsets of the rows in the packed buffer, flat over the batch (their running lengths).  The
        first call packs the rows on the device and leaves them there; later calls copy."""
        self._open()
        n = int(self.L.ka_sum_fam_ungapped_size(self.h))
        if n < 0:
            raise KalignAmdError(self.L.ka_last_error().decode())
        buf = np.zeros(max(n, 1), np.uint8)
        off = np.zeros(int(self.first[-1]) + 1, np.int64)
        self.ctx._chk(self.L.ka_sum_fam_ungapped(self.h, _ptr(buf), n, _ptr(off)))
        data = buf[:n].tobytes()
        rows = [[data[off[r]:off[r + 1]] for r in range(self.first[f], self.first[f + 1])] for f in range(len(self.sizes))]
        return (rows, off) if want_offsets else rows

    def gap_stats(self):
        """ka_sum_fam_gap_stats: device ms of the row and gappy passes and of the ungap pass; kernel launches and host
        synchronisations of the computation of the gaps and of the ungapped rows (zeros before; unchanged by copies)"""
        self._open()
        st = np.zeros(len(GAP_STATS), np.float64)
        self.ctx._chk(self.L.ka_sum_fam_gap_stats(self.h, _ptr(st)))
        return {k: (float(v) if k.endswith("_ms") else int(v)) for k, v in zip(GAP_STATS, st)}


def gap_values(counts):
    """ka_sum_fam_gap_values: the seven doubles of each family from its eight exact counts (int64 [n, 8], GAP_COUNTS) -- on
    the host alone.  float64 [n, 7] (GAP_VALUES)."""
    L = load_library()
    counts = np.ascontiguousarray(counts, np.int64).reshape(-1, len(GAP_COUNTS))
    values = np.zeros((len(counts), len(GAP_VALUES)), np.float64)
    if L.ka_sum_fam_gap_values(len(counts), _ptr(counts), _ptr(values)) != 0:
        raise KalignAmdError(L.ka_last_error().decode())
    return values


def _sum_fam_create(self, families_rows, gap=b"-"):
    """ka_sum_fam_create: a FamilySummary holding the rows of every family on this context's device"""
    return FamilySummary(self, families_rows, gap)


Context.family_summary = _sum_fam_create


IN_SEQ = ("residues", "gap_characters", "dropped", "checksum")
IN_FAM = ("biotype", "aligned", "min_len", "max_len", "no_code")
IN_STATS = ("scan_ms", "encode_ms", "launches", "syncs", "bytes", "run_wall_ms")
IN_TABLES = ("nucleotide", "reduced_protein", "protein")


def _pack_text(seqs):
    """a flat list of bytes -> (uint8 text, int64 offsets [n + 1])"""
    off = np.zeros(len(seqs) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.int64)
    text = np.frombuffer(b"".join(seqs), np.uint8)
    return (np.ascontiguousarray(text) if len(text) else np.zeros(1, np.uint8)), off


def _raw(s):
    """a sequence or a name as bytes: a str is its latin-1 bytes, one per character (a character past 255 is refused)"""
    try:
        return s.encode("latin-1") if isinstance(s, str) else bytes(s)
    except UnicodeEncodeError as e:
        raise KalignAmdError("a sequence holds a character that is no byte: %s" % e)


def input_tables():
    """ka_in_tables (no GPU): int8 [3, 128] -- nucleotides, reduced protein, protein (IN_TABLES); -1: no code"""
    L = load_library()
    t = np.zeros((3, 128), np.int8)
    if L.ka_in_tables(_ptr(t)) != 0:
        raise KalignAmdError(L.ka_last_error().decode())
    return t


def input_detect(freq):
    """ka_in_detect (no GPU): the biotype (0 protein, 1 DNA) of a 128-bin byte histogram"""
    L = load_library()
    f = np.ascontiguousarray(freq, np.int64)
    if f.shape != (128,):
        raise KalignAmdError("input_detect: a histogram has 128 bins")
    out = C.c_int(-1)
    if L.ka_in_detect(_ptr(f), C.byref(out)) != 0:
        raise KalignAmdError(L.ka_last_error().decode())
    return out.value


def input_order(sizes, residues, names=None):
    """ka_in_order (no GPU): sorted position -> input index, batch-wide, for families of `sizes` sequences with `residues`
    letters each; names: a flat list (bytes / str), one per sequence, or None"""
    L = load_library()
    first = _fam_first(sizes)
    res = np.ascontiguousarray(residues, np.int32)
    if len(res) != int(first[-1]) or (names is not None and len(names) != len(res)):
        raise KalignAmdError("input_order: one residue count (and one name) per sequence")
    nm, noff = _pack_text([_raw(x) for x in names]) if names is not None else (None, None)
    out = np.zeros(max(len(res), 1), np.int32)
    if L.ka_in_order(len(sizes), _ptr(first), _ptr(res), _ptr(nm), _ptr(noff), _ptr(out)) != 0:
        raise KalignAmdError(L.ka_last_error().decode())
    return out[:len(res)]


class FamilyInput(_CtxChild):
    """A batch of families from raw text (ka_in_fam): families is a list of lists of sequences (bytes / str) as a user has
    them -- mixed case, ambiguity codes, possibly aligned already.  Letters are residues, punctuation is gap characters (counted,
    then discarded), everything else below 128 is dropped; a byte >= 128 or a sequence without a letter is refused.  names: a
    list of lists like families, or None; biotype: None (detect every family), one value or one per family (-1: detect)."""
    _destroy = "ka_in_fam_destroy"

    def __init__(self, ctx, families, names=None, biotype=None):
        self.ctx, self.L = ctx, ctx.L
        if not ctx.h:
            raise KalignAmdError("the context is closed")
        fams = [[_raw(s) for s in f] for f in families]
        if not fams:
            raise KalignAmdError("a family input needs a family")
        self.sizes = [len(f) for f in fams]
        self.first = _fam_first(self.sizes)
        text, off = _pack_text([s for f in fams for s in f])
        nm = noff = None
        if names is not None:
            if [len(f) for f in names] != self.sizes:
                raise KalignAmdError("one name per sequence")
            nm, noff = _pack_text([_raw(x) for f in names for x in f])
        bt = None
        if biotype is not None:
            bt = np.ascontiguousarray(np.broadcast_to(np.asarray(biotype, np.int32), (len(fams),)))
        h = C.c_void_p()
        ctx._chk(self.L.ka_in_fam_create(ctx.h, len(fams), _ptr(self.first), _ptr(text), _ptr(off), _ptr(nm), _ptr(noff), _ptr(bt), C.byref(h)))
        self._adopt(ctx, h)
        self.n = int(self.first[-1])

    def _open(self):
        if not self.h:
            raise KalignAmdError("the family input is closed")
        return len(self.sizes)

    def _per_family(self, a):
        return [a[self.first[f]:self.first[f + 1]] for f in range(len(self.sizes))]

    def sequences(self):
        """per family an int32 array [n_f, 4] in input order: residues, gap characters, dropped bytes, checksum (IN_SEQ)"""
        self._open()
        recs = np.zeros((max(self.n, 1), len(IN_SEQ)), np.int32)
        self.ctx._chk(self.L.ka_in_fam_sequences(self.h, _ptr(recs)))
        return self._per_family(recs[:self.n])

    def families(self, want_freq=False):
        """per family a dict of IN_FAM: biotype (0 protein, 1 DNA), aligned (1 unaligned, 2 aligned, 3 unknown), min_len,
        max_len, no_code (letters without a code); want_freq: also freq, the int64 histogram of its 128 byte values"""
        F = self._open()
        recs, freq = np.zeros((F, len(IN_FAM)), np.int32), np.zeros((F, 128), np.int64)
        self.ctx._chk(self.L.ka_in_fam_families(self.h, _ptr(recs), _ptr(freq) if want_freq else None))
        out = [{k: int(v) for k, v in zip(IN_FAM, r)} for r in recs]
        if want_freq:
            for d, f in zip(out, freq):
                d["freq"] = f
        return out

    def order(self):
        """per family: sorted position -> index of the sequence in the family as given"""
        self._open()
        o = np.zeros(max(self.n, 1), np.int32)
        self.ctx._chk(self.L.ka_in_fam_order(self.h, _ptr(o)))
        return [x - self.first[f] for f, x in enumerate(self._per_family(o[:self.n]))]

    def encoded(self):
        """one (tree_codes, codes, letters) per family, each a list of uint8 arrays in sorted order: what
        Context.run_families takes as it stands"""
        self._open()
        size = int(self.L.ka_in_fam_size(self.h))
        t, c, l = (np.zeros(max(size, 1), np.uint8) for _ in range(3))
        off, lens = np.zeros(max(self.n, 1), np.int32), np.zeros(max(self.n, 1), np.int32)
        self.ctx._chk(self.L.ka_in_fam_encoded(self.h, _ptr(t), _ptr(c), _ptr(l), _ptr(off), _ptr(lens)))
        out = []
        for f in range(len(self.sizes)):
            rng = range(int(self.first[f]), int(self.first[f + 1]))
            out.append(tuple([p[off[i]:off[i] + lens[i]].copy() for i in rng] for p in (t, c, l)))
        return out

    def run(self, biotype, subm, scal, n_anchors=0, weight=2.0, realign=0, refine=0, n_threads=4, gap=b"-"):
        """ka_in_fam_run: aligns the families of this biotype with its subm / scal, as run_families aligns them; their rows
        stay in the handle in input order"""
        self._open()
        sub = np.ascontiguousarray(subm, np.float32).reshape(-1)
        sc = np.ascontiguousarray(scal, np.float32)
        self.ctx._chk(self.L.ka_in_fam_run(self.h, int(biotype), _ptr(sub), _ptr(sc), int(n_anchors), float(weight), int(realign),
                                           int(n_threads), int(refine), gap[0]))

    def rows(self):
        """one list of rows (bytes) per family, in the caller's order; fails while a family has not been run"""
        F = self._open()
        need = int(self.L.ka_in_fam_rows_size(self.h))
        if need < 0:
            raise KalignAmdError(self.L.ka_last_error().decode())
        buf, widths = np.zeros(max(need, 1), np.uint8), np.zeros(F, np.int32)
        self.ctx._chk(self.L.ka_in_fam_rows(self.h, _ptr(buf), need, _ptr(widths)))
        return _unpack_families(buf, self.sizes, widths)

    def stats(self):
        """ka_in_fam_stats: device ms of the scan and of the encode, kernel launches and host synchronisations of the
        construction, the raw bytes, the wall ms of the run() calls so far (IN_STATS)"""
        self._open()
        st = np.zeros(len(IN_STATS), np.float64)
        self.ctx._chk(self.L.ka_in_fam_stats(self.h, _ptr(st)))
        return {k: (float(v) if k.endswith("_ms") else int(v)) for k, v in zip(IN_STATS, st)}


def _in_fam_create(self, families, names=None, biotype=None):
    """ka_in_fam_create: a FamilyInput over raw sequences on this context's device"""
    return FamilyInput(self, families, names, biotype)


Context.family_input = _in_fam_create


COD_SEQ = ("residues", "gap_characters", "dropped", "codons", "stops", "x_codons")
COD_STATS = ("pack_ms", "translate_ms", "back_ms", "launches", "syncs", "back_launches", "back_syncs", "bytes", "run_wall_ms")


def codon_table():
    """ka_cod_table (no GPU): the 64 letters of the standard code as bytes, index 16a + 4b + c with A 0, C 1, G 2, T 3; b"*": a stop"""
    L = load_library()
    t = np.zeros(64, np.uint8)
    if L.ka_cod_table(_ptr(t)) != 0:
        raise KalignAmdError(L.ka_last_error().decode())
    return t.tobytes()


class FamilyCodons(_CtxChild):
    """Coding DNA of a batch of families, aligned in frame (ka_cod_fam): families is a list of lists of sequences (bytes / str)
    under the input stage's byte rule, upper-cased; three residues a codon, the standard code over exactly A C G T (any other
    letter makes the codon X; U is not T), stop codons omitted wherever they stand.  A residue count that is no multiple of 3,
    a byte >= 128 and a sequence without a protein are refused.  run() aligns the proteins and backtranslates; back() takes
    protein rows the caller brings.  names: a list of lists like families, or None."""
    _destroy = "ka_cod_fam_destroy"

    def __init__(self, ctx, families, names=None):
        self.ctx, self.L = ctx, ctx.L
        if not ctx.h:
            raise KalignAmdError("the context is closed")
        fams = [[_raw(s) for s in f] for f in families]
        if not fams:
            raise KalignAmdError("a codon stage needs a family")
        self.sizes = [len(f) for f in fams]
        self.first = _fam_first(self.sizes)
        text, off = _pack_text([s for f in fams for s in f])
        nm = noff = None
        if names is not None:
            if [len(f) for f in names] != self.sizes:
                raise KalignAmdError("one name per sequence")
            nm, noff = _pack_text([_raw(x) for f in names for x in f])
        h = C.c_void_p()
        ctx._chk(self.L.ka_cod_fam_create(ctx.h, len(fams), _ptr(self.first), _ptr(text), _ptr(off), _ptr(nm), _ptr(noff), C.byref(h)))
        self._adopt(ctx, h)
        self.n = int(self.first[-1])

    def _open(self):
        if not self.h:
            raise KalignAmdError("the codon stage is closed")
        return len(self.sizes)

    def sequences(self):
        """per family an int32 array [n_f, 6] in input order: residues, gap characters, dropped bytes, codons, stop codons, X
        codons (COD_SEQ)"""
        self._open()
        recs = np.zeros((max(self.n, 1), len(COD_SEQ)), np.int32)
        self.ctx._chk(self.L.ka_cod_fam_sequences(self.h, _ptr(recs)))
        return [recs[self.first[f]:self.first[f + 1]] for f in range(len(self.sizes))]

    def proteins(self):
        """per family its translated proteins (bytes) in input order"""
        self._open()
        size = int(self.L.ka_cod_fam_protein_size(self.h))
        buf, off = np.zeros(max(size, 1), np.uint8), np.zeros(self.n + 1, np.int64)
        self.ctx._chk(self.L.ka_cod_fam_protein(self.h, _ptr(buf), _ptr(off)))
        return [[buf[off[i]:off[i + 1]].tobytes() for i in range(int(self.first[f]), int(self.first[f + 1]))] for f in range(len(self.sizes))]

    def run(self, subm, scal, n_anchors=0, weight=2.0, realign=0, refine=0, n_threads=4, gap=b"-"):
        """ka_cod_fam_run: aligns the proteins with the protein's subm / scal, as FamilyInput.run aligns them, and
        backtranslates their rows; protein rows and codon rows stay in the handle in input order"""
        self._open()
        sub = np.ascontiguousarray(subm, np.float32).reshape(-1)
        sc = np.ascontiguousarray(scal, np.float32)
        self.ctx._chk(self.L.ka_cod_fam_run(self.h, _ptr(sub), _ptr(sc), int(n_anchors), float(weight), int(realign), int(n_threads),
                                            int(refine), gap[0]))

    def back(self, protein_rows, gap=b"-"):
        """ka_cod_fam_back: backtranslates one list of protein rows per family (rows in input order); a row whose residues
        are not as many as its sequence's non-stop codons is refused"""
        F = self._open()
        if len(protein_rows) != F or [len(f) for f in protein_rows] != self.sizes:
            raise KalignAmdError("one protein row per sequence")
        packed, widths = pack_families(protein_rows)
        self.ctx._chk(self.L.ka_cod_fam_back(self.h, _ptr(np.ascontiguousarray(packed)), len(packed), _ptr(widths), gap[0]))

    def _rows(self, name):
        F = self._open()
        need = int(getattr(self.L, name + "_size")(self.h))
        if need < 0:
            raise KalignAmdError(self.L.ka_last_error().decode())
        buf, widths = np.zeros(max(need, 1), np.uint8), np.zeros(F, np.int32)
        self.ctx._chk(getattr(self.L, name)(self.h, _ptr(buf), need, _ptr(widths)))
        return _unpack_families(buf, self.sizes, widths)

    def rows(self):
        """one list of codon rows (bytes) per family, in the caller's order; fails before a run() or a back()"""
        return self._rows("ka_cod_fam_rows")

    def protein_rows(self):
        """the protein rows the codon rows were made from, the same way"""
        return self._rows("ka_cod_fam_protein_rows")

    def stats(self):
        """ka_cod_fam_stats: device ms of the pack, the translate and the last backtranslation; kernel launches and host
        synchronisations of the construction and of the last backtranslation; the raw bytes; the wall ms of the run() calls
        so far (COD_STATS)"""
        self._open()
        st = np.zeros(len(COD_STATS), np.float64)
        self.ctx._chk(self.L.ka_cod_fam_stats(self.h, _ptr(st)))
        return {k: (float(v) if k.endswith("_ms") else int(v)) for k, v in zip(COD_STATS, st)}


def _cod_fam_create(self, families, names=None):
    """ka_cod_fam_create: a FamilyCodons over raw coding sequences on this context's device"""
    return FamilyCodons(self, families, names)


Context.family_codons = _cod_fam_create


OUT_STATS = ("rows_ms", "fill_ms", "launches", "syncs")
# write_msa_clu's header with the version the reference of this tree's oracle/_ref build writes (tests/golden/out_*.npz pin it)
CLUSTAL_HEADER = b"Kalign (3.5.1) multiple sequence alignment"
MSF_DATE = "%B %d, %Y %H:%M"       # write_msa_msf's strftime format


def pp_char(confidence):
    """ka_out_pp_char (no GPU): the Stockholm PP byte of a confidence (its float32 value) as bytes, or None for a NaN and a
    value outside [0, 1]"""
    c = int(load_library().ka_out_pp_char(float(np.float32(confidence))))
    return None if c < 0 else bytes([c])


def _pack_names(names, sizes):
    if names is None:
        return None, None
    if [len(f) for f in names] != list(sizes):
        raise KalignAmdError("one name per sequence")
    return _pack_text([_raw(x) for f in names for x in f])


def output_check(families_rows, names=None):
    """ka_out_fam_check (no GPU): raises with the library's message when the batch or a name is refused"""
    L = load_library()
    fams = [[_raw(x) for x in f] for f in families_rows]
    sizes = [len(f) for f in fams]
    rows, widths = pack_families(fams)
    nm, noff = _pack_names(names, sizes)
    if L.ka_out_fam_check(len(fams), _ptr(_fam_first(sizes)), _ptr(rows if len(rows) else np.zeros(1, np.uint8)), _ptr(widths), _ptr(nm), _ptr(noff)) != 0:
        raise KalignAmdError(L.ka_last_error().decode())


def output_sizes(sizes, widths, name_lens, fmt, param):
    """ka_out_fam_text_sizes (no GPU): the bytes of every family's text from the closed forms.  sizes, widths: per family;
    name_lens: a list of lists of name lengths, or None (the default names); fmt "fasta" (param line_length), "clustal" (param
    the header's bytes) or "stockholm" (param 1 residue, 2 column, 3 both confidences)"""
    L = load_library()
    noff = None
    if name_lens is not None:
        noff = np.zeros(int(sum(sizes)) + 1, np.int64)
        noff[1:] = np.cumsum([n for f in name_lens for n in f], dtype=np.int64)
    off = np.zeros(len(sizes) + 1, np.int64)
    if L.ka_out_fam_text_sizes(len(sizes), _ptr(_fam_first(sizes)), _ptr(np.ascontiguousarray(widths, np.int32)), _ptr(noff),
                               ("fasta", "clustal", "stockholm").index(fmt), int(param), _ptr(off)) != 0:
        raise KalignAmdError(L.ka_last_error().decode())
    return np.diff(off)


class FamilyOutput(_CtxChild):
    """The finished rows of a batch of families on the device (ka_out_fam) and the text the reference's writers make of each --
    write_msa_fasta / kalign.io.write_fasta, write_msa_clu, write_msa_msf, kalign.io.write_stockholm with PP lines -- byte
    for byte, each format in one launch whatever the number of families.  families_rows: one list of rows per family;
    names: a list of lists like it (1 to 255 printable bytes each), or None: seq0, seq1, ... per family; gap: the gap byte.
    Every writer returns a list of bytes, one text per family."""
    _destroy = "ka_out_fam_destroy"

    def __init__(self, ctx, families_rows, names=None, gap=b"-"):
        self.ctx, self.L = ctx, ctx.L
        if not ctx.h:
            raise KalignAmdError("the context is closed")
        fams = [[_raw(x) for x in f] for f in families_rows]
        if not fams:
            raise KalignAmdError("a family output needs a family")
        gap = gap.encode() if isinstance(gap, str) else bytes(gap)
        if len(gap) != 1:
            raise KalignAmdError("the gap is one byte")
        self.sizes = [len(f) for f in fams]
        self.first = _fam_first(self.sizes)
        rows, self.widths = pack_families(fams)
        nm, noff = _pack_names(names, self.sizes)
        h = C.c_void_p()
        ctx._chk(self.L.ka_out_fam_create(ctx.h, len(fams), _ptr(self.first), _ptr(rows if len(rows) else np.zeros(1, np.uint8)),
                                          _ptr(self.widths), gap[0], _ptr(nm), _ptr(noff), C.byref(h)))
        self._adopt(ctx, h)
        self.n = int(self.first[-1])

    def _open(self):
        if not self.h:
            raise KalignAmdError("the family output is closed")
        return len(self.sizes)

    def _texts(self, size, write, cap=None):
        """the batch's text through write(buf, cap, fam_off), cut per family; cap: a cap other than the size (tests)"""
        if size < 0:
            raise KalignAmdError(self.L.ka_last_error().decode())
        cap = size if cap is None else cap
        buf, off = np.zeros(max(cap, 1), np.uint8), np.zeros(len(self.sizes) + 1, np.int64)
        self.ctx._chk(write(_ptr(buf), cap, _ptr(off)))
        raw = buf.tobytes()
        return [raw[off[f]:off[f + 1]] for f in range(len(self.sizes))]

    def fasta(self, line_length=60, cap=None):
        """per family ">name" and the row in lines of line_length bytes: 60 is write_msa_fasta, 80 kalign.io.write_fasta"""
        self._open()
        L = int(line_length)
        return self._texts(int(self.L.ka_out_fam_fasta_size(self.h, L)), lambda b, c, o: self.L.ka_out_fam_fasta(self.h, L, b, c, o), cap)

    def clustal(self, header=CLUSTAL_HEADER, cap=None):
        """write_msa_clu's text per family under `header`"""
        self._open()
        hd = _raw(header)
        return self._texts(int(self.L.ka_out_fam_clustal_size(self.h, hd)), lambda b, c, o: self.L.ka_out_fam_clustal(self.h, hd, b, c, o), cap)

    def msf_records(self):
        """per family (int32 [n_f, 2]: characters and prefix checksum of every row, the family's check)"""
        F = self._open()
        recs, check = np.zeros((max(self.n, 1), 2), np.int32), np.zeros(F, np.int32)
        self.ctx._chk(self.L.ka_out_fam_msf_records(self.h, _ptr(recs), _ptr(check)))
        return [(recs[self.first[f]:self.first[f + 1]], int(check[f])) for f in range(F)]

    def msf(self, titles, biotypes, date=None, cap=None):
        """write_msa_msf's text per family.  titles: one per family (the file's basename, or "stdout"); biotypes: 0 protein /
        1 DNA, one value or one per family; date: write_msa_msf's date string (MSF_DATE), now when None"""
        F = self._open()
        if len(titles) != F:
            raise KalignAmdError("%d titles for %d families" % (len(titles), F))
        if date is None:
            import time
            date = time.strftime(MSF_DATE)
        t, toff = _pack_text([_raw(x) for x in titles])
        bt = np.ascontiguousarray(np.broadcast_to(np.asarray(biotypes, np.int32), (F,)))
        d = _raw(date)
        return self._texts(int(self.L.ka_out_fam_msf_size(self.h, _ptr(t), _ptr(toff), _ptr(bt), d)),
                           lambda b, c, o: self.L.ka_out_fam_msf(self.h, _ptr(t), _ptr(toff), _ptr(bt), d, b, c, o), cap)

    def _conf(self, conf, per_row, what):
        """per family confidences -> one float32 array; float64 values that float32 does not hold are refused"""
        if conf is None:
            return None
        F = len(self.sizes)
        if len(conf) != F:
            raise KalignAmdError("%d %s confidences for %d families" % (len(conf), what, F))
        parts = []
        for f, c in enumerate(conf):
            a = np.asarray(c)
            want = (self.sizes[f], int(self.widths[f])) if per_row else (int(self.widths[f]),)
            if a.shape != want:
                raise KalignAmdError("family %d: %s confidences of shape %s, not %s" % (f, what, a.shape, want))
            b = a
            if a.dtype != np.float32:
                a64 = np.asarray(a, np.float64)
                with np.errstate(over="ignore"):
                    b = a64.astype(np.float32)
                ok = (b.astype(np.float64) == a64) | np.isnan(a64)
                if not ok.all():
                    k = tuple(int(x) for x in np.argwhere(~ok)[0])
                    raise KalignAmdError("family %d: %s confidence at %s is not a float32 value (%r): a rounding across 0.95 or a tenth would "
                                         "change a PP byte; round it yourself" % (f, what, k, float(a64[k])))
            parts.append(b.reshape(-1))
        return np.ascontiguousarray(np.concatenate(parts))

    def stockholm(self, residue_confidence=None, column_confidence=None, cap=None):
        """kalign.io.write_stockholm's text per family with "#=GR <name> PP" lines (residue_confidence: per family [n_f, W_f])
        and / or a "#=GC PP_cons" line (column_confidence: per family [W_f]); one of the two at least"""
        self._open()
        res, col = self._conf(residue_confidence, True, "residue"), self._conf(column_confidence, False, "column")
        return self._texts(int(self.L.ka_out_fam_stockholm_size(self.h, res is not None, col is not None)),
                           lambda b, c, o: self.L.ka_out_fam_stockholm(self.h, _ptr(res), _ptr(col), b, c, o), cap)

    def stats(self):
        """ka_out_fam_stats: device ms of the MSF row pass and of the last fill; kernel launches and host synchronisations of
        the last writer (OUT_STATS)"""
        self._open()
        st = np.zeros(len(OUT_STATS), np.float64)
        self.ctx._chk(self.L.ka_out_fam_stats(self.h, _ptr(st)))
        return {k: (float(v) if k.endswith("_ms") else int(v)) for k, v in zip(OUT_STATS, st)}


def _out_fam_create(self, families_rows, names=None, gap=b"-"):
    """ka_out_fam_create: a FamilyOutput holding rows and names of every family on this context's device"""
    return FamilyOutput(self, families_rows, names, gap)


Context.family_output = _out_fam_create


def ens_fam_consensus_host(fam_lens, cands, families_letters, n_threads=1):
    """tests only: ka_debug_ens_fam_consensus_host -- the greedy union, column order and fill of every family over given
    candidate lists (cands[f]: int array [n, 2], residue numbers flat inside the family), dealt to n_threads as
    FamilyEnsemble.consensus deals them; no GPU needed.  Returns one list of rows per family."""
    L = load_library()
    sizes = [len(l) for l in fam_lens]
    first = _fam_first(sizes)
    lens = np.ascontiguousarray(np.concatenate([np.asarray(l, np.int32).reshape(-1) for l in fam_lens]), np.int32)
    cfirst = np.zeros(len(sizes) + 1, np.int64)
    cfirst[1:] = np.cumsum([len(c) for c in cands])
    parts = [np.asarray(c, np.int32).reshape(-1, 2) for c in cands]
    cand = np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros((0, 2), np.int32), np.int32)
    flat = np.frombuffer(b"".join(x.encode() if isinstance(x, str) else bytes(x) for f in families_letters for x in f), np.uint8)
    w = np.zeros(len(sizes), np.int32)
    cap = int(sum(n * (int(np.sum(l)) + 1) for n, l in zip(sizes, fam_lens)))         # (no more columns than residues)
    buf = np.zeros(max(cap, 1), np.uint8)
    if L.ka_debug_ens_fam_consensus_host(len(sizes), _ptr(first), _ptr(lens), _ptr(cfirst), _ptr(cand if len(cand) else np.zeros((1, 2), np.int32)),
                                         _ptr(flat if len(flat) else np.zeros(1, np.uint8)), int(n_threads), _ptr(w), _ptr(buf), cap):
        raise KalignAmdError(L.ka_last_error().decode())
    return _unpack_families(buf, sizes, w)


def guide_tree_from(lens, dist, n_threads=1, dm_scale=None):
    """build_tree_kmeans with the caller's distance source (ka_guide_tree_from; host only, no GPU needed):
    dist(ia, ib) -> calc_distance of every pair, as an int array."""
    L = load_library()
    lens = np.ascontiguousarray(lens, np.int32)

    def cb(_user, n, ia, ib, out):
        try:
            d = dist(np.ctypeslib.as_array(ia, (n,)).copy(), np.ctypeslib.as_array(ib, (n,)).copy())
            np.ctypeslib.as_array(out, (n,))[:] = d
            return 0
        except Exception:                     # reported as "the distance source failed"
            return 1

    tasks = np.zeros((len(lens) - 1, 3), np.int32)
    sd = np.zeros(len(lens), np.float32)
    sc = _dm_scale(dm_scale, len(lens))
    if L.ka_guide_tree_from(len(lens), _ptr(lens), DIST_FN(cb), None, int(n_threads), _ptr(sc), _ptr(tasks), _ptr(sd)):
        raise KalignAmdError(L.ka_last_error().decode())
    return tasks, sd


def guide_forest_from(fam_lens, dist, n_threads=1, dm_scale=None):
    """ka_guide_forest_from: the guide trees of a batch of families with the caller's distance source (host only, no GPU
    needed).  fam_lens: one array of sequence lengths per family; dist(ia, ib) gets GLOBAL sequence indices (families
    concatenated) and is called at most twice.  Returns (tasks in the forest's numbering, seq_distances)."""
    L = load_library()
    sizes = [len(x) for x in fam_lens]
    lens = np.ascontiguousarray(np.concatenate([np.asarray(x, np.int32).reshape(-1) for x in fam_lens]), np.int32)
    first = _fam_first(sizes)

    def cb(_user, n, ia, ib, out):
        try:
            d = dist(np.ctypeslib.as_array(ia, (n,)).copy(), np.ctypeslib.as_array(ib, (n,)).copy())
            np.ctypeslib.as_array(out, (n,))[:] = d
            return 0
        except Exception:                     # reported as "the distance source failed"
            return 1

    tasks = np.zeros((max(len(lens) - len(sizes), 1), 3), np.int32)
    sd = np.zeros(len(lens), np.float32)
    sc = _dm_scale_forest(dm_scale, sizes)
    nt = C.c_int(0)
    if L.ka_guide_forest_from(len(sizes), _ptr(first), _ptr(lens), DIST_FN(cb), None, int(n_threads), _ptr(sc), _ptr(tasks), C.byref(nt), _ptr(sd)):
        raise KalignAmdError(L.ka_last_error().decode())
    return tasks[:nt.value], sd


def guide_last_bisect():
    """(milliseconds, ran on the device) of the 2-means bisection inside the last ka_guide_tree of this process"""
    L = load_library()
    on = C.c_int(0)
    ms = float(L.ka_guide_last_bisect_ms(C.byref(on)))
    return ms, bool(on.value)


def weave_gaps(lens, recs, paths):
    """Host-only make_seq/update_gaps over all tasks in tree order (ka_weave_gaps); needs the library but no GPU.
    recs: sequence of TaskRec in task order with path_off into `paths`.  Returns the gap array per sequence."""
    L = load_library()
    lens = np.ascontiguousarray(lens, np.int32)
    arr = (TaskRec * len(recs))(*recs)
    paths = np.ascontiguousarray(paths, np.int32)
    gaps = np.zeros(int(lens.sum()) + len(lens), np.int32)
    if L.ka_weave_gaps(len(lens), _ptr(lens), len(recs), arr, _ptr(paths), _ptr(gaps)):
        raise KalignAmdError(L.ka_last_error().decode())
    out, o = [], 0
    for n in lens:
        out.append(gaps[o:o + int(n) + 1].copy())
        o += int(n) + 1
    return out


def msa_tree(codes, tasks, subm, scal, seq_distances=None, flags=0, device=0):
    ctx = Context(device)
    try:
        return ctx.msa_tree(codes, tasks, subm, scal, seq_distances, flags)
    finally:
        ctx.close()


def pairwise_batch(codes, ia, ib, subm, gpo, gpe, tgpe, device=0):
    ctx = Context(device)
    try:
        return ctx.pairwise_batch(codes, ia, ib, subm, gpo, gpe, tgpe)
    finally:
        ctx.close()


def dist_plan_subtrees(lens, tasks, world):
    """ka_dist_plan_subtrees: (run_rank[n_tasks], top task ids) -- pure host logic, needs no GPU"""
    L = load_library()
    lens = np.ascontiguousarray(lens, np.int32)
    tasks = np.ascontiguousarray(tasks, np.int32)
    run_rank = np.zeros(len(tasks), np.int32)
    top = np.zeros(len(tasks), np.int32)
    n_top = C.c_int(0)
    if L.ka_dist_plan_subtrees(len(lens), _ptr(lens), len(tasks), _ptr(tasks), int(world), _ptr(run_rank), _ptr(top), C.byref(n_top)):
        raise RuntimeError(L.ka_last_error().decode())
    return run_rank, top[:n_top.value].tolist()


PLAN_SCALARS = ("levels", "n_blocks", "max_cluster", "n_trees", "chain_level", "queue_first", "queue_off", "queue_n", "overlap_plan",
                "chain_blocks_off", "chain_blocks_n")
PLAN_TASK_FIELDS = ("parent", "chain_need", "is_root", "wait_mult", "qa", "qb")


def _flat_plan(L, n_tasks, n_cus, call):
    """one flattened launch plan (ka_debug_plan / ka_debug_ctx_plan) as a dict: the PLAN_SCALARS as ints, the PLAN_TASK_FIELDS
    as int32[n_tasks], blocks int32[n, 2], blocks_off, level_lean"""
    scalars, per_task = np.zeros(16, np.int32), np.zeros((len(PLAN_TASK_FIELDS), n_tasks), np.int32)
    blocks_off, level_lean = np.zeros(n_tasks + 1, np.int32), np.zeros(n_tasks, np.int32)
    cap = 4 * n_tasks + 8 * n_cus + 4096
    for _ in range(2):
        blocks = np.zeros((cap, 2), np.int32)
        rc = call(_ptr(scalars), _ptr(per_task), _ptr(blocks), cap, _ptr(blocks_off), _ptr(level_lean))
        if not rc or scalars[1] <= cap:
            break
        cap = int(scalars[1])                           # (a deep, narrow tree: every level a table of its own)
    if rc:
        raise KalignAmdError(L.ka_last_error().decode())
    plan = {k: int(v) for k, v in zip(PLAN_SCALARS, scalars)}
    plan.update({k: per_task[i].copy() for i, k in enumerate(PLAN_TASK_FIELDS)})
    plan.update(blocks=blocks[:plan["n_blocks"]].copy(), blocks_off=blocks_off[:plan["levels"] + 1].copy(),
                level_lean=level_lean[:plan["levels"]].copy())
    return plan


def debug_plan(lens, tasks, n_cus, shared=False, cons_K=0, hooks=0, task_ids=None):
    """ka_debug_plan: the launch plan of a job on a device of n_cus compute units, under the KA_* switches the environment holds
    now -- pure host logic, needs no GPU"""
    L = load_library()
    lens = np.ascontiguousarray(lens, np.int32)
    tasks = np.ascontiguousarray(tasks, np.int32)
    ids = None if task_ids is None else np.ascontiguousarray(task_ids, np.int32)
    return _flat_plan(L, len(tasks), int(n_cus), lambda *out: L.ka_debug_plan(
        len(lens), _ptr(lens), len(tasks), _ptr(tasks), int(n_cus), int(bool(shared)), int(cons_K), int(hooks),
        _ptr(ids) if ids is not None else None, 0 if ids is None else len(ids), *out))


def dist_unique_id():
    """rank 0: the 128 bytes every rank hands to Dist (ncclGetUniqueId)"""
    L = load_library()
    buf = np.zeros(128, np.uint8)
    if L.ka_dist_unique_id(_ptr(buf)):
        raise RuntimeError(L.ka_last_error().decode())
    return buf


class Dist:
    """Thin caller of the C multi-GPU layer (ka_dist_*): ONE alignment over the GPUs of a node, RCCL driven from C.
    unique_id: the 128 bytes of dist_unique_id() from rank 0 (None with world == 1: no communicator)."""

    def __init__(self, ctx, rank, world, unique_id=None, loopback=None):
        self.ctx, self.L = ctx, ctx.L
        self.h = C.c_void_p()
        if loopback is not None:                      # tests: threads of one process (ka_dist_loopback_new)
            rc = self.L.ka_dist_create_loopback(ctx.h, int(rank), int(world), loopback, C.byref(self.h))
        else:
            uid = None if unique_id is None else np.ascontiguousarray(unique_id, np.uint8)
            rc = self.L.ka_dist_create(ctx.h, int(rank), int(world), _ptr(uid) if uid is not None else None, C.byref(self.h))
        if rc:
            raise RuntimeError(self.L.ka_last_error().decode())

    def _chk(self, rc):
        if rc:
            raise RuntimeError(self.L.ka_last_error().decode())

    def plan(self):
        self._chk(self.L.ka_dist_plan(self.h))

    def get_plan(self):
        n = self.ctx._job["ntasks"]
        run_rank, top = np.zeros(n, np.int32), np.zeros(n, np.int32)
        n_top, n_moves = C.c_int(0), C.c_int(0)
        self._chk(self.L.ka_dist_get_plan(self.h, _ptr(run_rank), _ptr(top), C.byref(n_top), C.byref(n_moves)))
        return run_rank, top[:n_top.value].tolist(), n_moves.value

    def consistency(self, n_anchors, weight):
        self._chk(self.L.ka_dist_consistency(self.h, int(n_anchors), float(weight)))

    def tree_run(self):
        self._chk(self.L.ka_dist_tree_run(self.h))

    def download(self):
        n = self.ctx._job["ntasks"]
        recs = (TaskRec * n)()
        cap = int(self.L.ka_dist_paths_size(self.h))
        paths = np.zeros(max(cap, 1), np.int32)
        used = C.c_longlong(0)
        self._chk(self.L.ka_dist_download(self.h, recs, _ptr(paths), cap, C.byref(used)))
        return list(recs), paths[:used.value]

    def last_ms(self):
        return float(self.L.ka_dist_last_ms(self.h))

    def retries(self):
        return int(self.L.ka_dist_retries(self.h))

    def close(self):
        if self.h:
            self.L.ka_dist_destroy(self.h)
            self.h = C.c_void_p()


class Multi:
    """ka_multi_*: the GPUs of one node under one caller -- one context and one rank of the sharded path per device, the ranks
    as threads inside the library.  loopback=True: every rank on device 0 over the in-process transport (one-GPU boxes)."""

    def __init__(self, world, loopback=False, devices=None):
        self.L = load_library()
        self.h = C.c_void_p()
        dev = None if devices is None else np.ascontiguousarray(devices, np.int32)
        if self.L.ka_multi_create(int(world), _ptr(dev) if dev is not None else None, 1 if loopback else 0, C.byref(self.h)):
            raise RuntimeError(self.L.ka_multi_last_error().decode())
        self._job = None

    def _chk(self, rc):
        if rc:
            raise RuntimeError(self.L.ka_multi_last_error().decode())

    def _args(self, codes, tasks, subm, scal, seq_distances):
        flat, off, lens = _flatten(codes)
        tasks = np.ascontiguousarray(tasks, np.int32)
        sd = np.ascontiguousarray(seq_distances, np.float32)
        sub = np.ascontiguousarray(subm, np.float32).reshape(-1)
        sc = np.ascontiguousarray(scal, np.float32)
        self._job = {"lens": lens, "ntasks": len(tasks), "keep": (flat, off, lens, tasks, sd, sub, sc)}
        return flat, off, lens, tasks, sd, sub, sc

    def consistency(self, codes, tasks, subm, scal, seq_distances, n_anchors, weight):
        flat, off, lens, tasks, sd, sub, sc = self._args(codes, tasks, subm, scal, seq_distances)
        ids = np.zeros(max(n_anchors, 1), np.int32)
        maps = np.zeros(int(lens.sum()) * max(n_anchors, 1) + 1, np.int32)
        k = self.L.ka_multi_consistency(self.h, len(lens), _ptr(flat), _ptr(off), _ptr(lens), _ptr(sd), len(tasks), _ptr(tasks),
                                        _ptr(sub), _ptr(sc), 0, int(n_anchors), float(weight), _ptr(ids), _ptr(maps))
        if k < 0:
            raise RuntimeError(self.L.ka_multi_last_error().decode())
        return ids[:k], maps[:int(lens.sum()) * k]

    def tree_run(self, codes, tasks, subm, scal, seq_distances, n_anchors=0, weight=0.0, keep_consistency=False):
        flat, off, lens, tasks, sd, sub, sc = self._args(codes, tasks, subm, scal, seq_distances)
        self._chk(self.L.ka_multi_tree_run(self.h, len(lens), _ptr(flat), _ptr(off), _ptr(lens), _ptr(sd), len(tasks), _ptr(tasks),
                                           _ptr(sub), _ptr(sc), FLAG_KEEP_CONSISTENCY if keep_consistency else 0, int(n_anchors), float(weight)))

    def download(self):
        lens, n = self._job["lens"], self._job["ntasks"]
        recs = (TaskRec * n)()
        cap = int(self.L.ka_multi_paths_size(self.h))
        paths = np.zeros(max(cap, 1), np.int32)
        gaps = np.zeros(int(lens.sum()) + len(lens), np.int32)
        self._chk(self.L.ka_multi_download(self.h, len(lens), _ptr(lens), n, recs, _ptr(paths), cap, _ptr(gaps)))
        out, g = [], 0
        for ln in lens:
            out.append(gaps[g:g + int(ln) + 1].copy())
            g += int(ln) + 1
        return list(recs), paths, out

    def runs(self):
        return int(self.L.ka_multi_runs(self.h))

    def ctx(self, rank=0):
        """rank's single-GPU context as a borrowed Context (ka_multi_ctx)"""
        h = self.L.ka_multi_ctx(self.h, int(rank))
        if not h:
            raise RuntimeError("ka_multi_ctx: bad rank")
        flat, off, lens, tasks, sd, sub, sc = self._job["keep"]
        return Context.borrowed(h, job=dict(lens=lens, ntasks=len(tasks), n=len(lens)))

    def adopt(self, recs, gaps):
        """ka_multi_adopt: rank 0's context takes the alignment of the last sharded run over"""
        arr = (TaskRec * len(recs))(*recs)
        flat = np.ascontiguousarray(np.concatenate([np.asarray(g, np.int32) for g in gaps]), np.int32)
        self._chk(self.L.ka_multi_adopt(self.h, arr, _ptr(flat)))

    def close(self):
        if self.h:
            self.L.ka_multi_destroy(self.h)
            self.h = C.c_void_p()
