"""ctypes binding of libgbrs_hip.so (include/gbrs_hip.h).

There is no CPU fallback: importing this module without the built library, or calling into
it without a visible gfx950 device, raises.  Build with ``python -c "import __graft_entry__ as g;
g.build()"``.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# GBRS_TUNING_LIB: a variant build of the same library (scripts/build_variant.sh), for A/B runs of kernel experiments
LIB_PATH = os.environ.get("GBRS_TUNING_LIB") or os.path.join(_HERE, "libgbrs_hip.so")

# names every build must export (checked by tests/test_abi.py against include/gbrs_hip.h)
EXPORTS = [
    "gbrs_last_error", "gbrs_abi_version", "gbrs_device_count", "gbrs_warm_up",
    "gbrs_em_create", "gbrs_em_create_device", "gbrs_em_create_masked", "gbrs_em_create_masked_device", "gbrs_em_set_initial_values", "gbrs_em_prepare", "gbrs_em_step", "gbrs_em_run",
    "gbrs_em_set_groups", "gbrs_em_step_model", "gbrs_em_posterior",
    "gbrs_em_resample", "gbrs_em_weights", "gbrs_em_resample_info",
    "gbrs_em_bootstrap_begin", "gbrs_em_bootstrap_add", "gbrs_em_bootstrap_get",
    "gbrs_em_get", "gbrs_em_set_theta", "gbrs_em_group_sums", "gbrs_em_estep_partial",
    "gbrs_em_finish_step", "gbrs_em_prepare_partial", "gbrs_em_finish_prepare", "gbrs_em_stream",
    "gbrs_em_set_stream",
    "gbrs_em_sync", "gbrs_em_pair_begin", "gbrs_em_pair_check", "gbrs_em_pair_status", "gbrs_em_info", "gbrs_em_fold_counts", "gbrs_em_tile_cut", "gbrs_em_gather_mstep", "gbrs_em_tile_shapes", "gbrs_em_stripe_census",
    "gbrs_alignment_counts",
    "gbrs_counts_create", "gbrs_counts_get", "gbrs_counts_destroy", "gbrs_em_destroy",
    "gbrs_shard_plan", "gbrs_shard_index", "gbrs_shard_gather",
    "gbrs_hmm_create", "gbrs_hmm_set_expression", "gbrs_hmm_set_eprob", "gbrs_hmm_run",
    "gbrs_hmm_get", "gbrs_hmm_info", "gbrs_hmm_destroy",
    "gbrs_grid_knots", "gbrs_hmm_set_grid", "gbrs_hmm_grid", "gbrs_hmm_grid_info", "gbrs_hmm_sample_paths", "gbrs_hmm_sample_info",
    "gbrs_hmm_diagnostics", "gbrs_hmm_pair_posterior", "gbrs_hmm_diagnostics_info",
    "gbrs_hmm_set_panel", "gbrs_hmm_match", "gbrs_hmm_match_info",
    "gbrs_hmm_set_snps", "gbrs_hmm_impute", "gbrs_hmm_impute_info", "gbrs_hmm_impute_times",
    "gbrs_hmm_loglik", "gbrs_hmm_loglik_tables", "gbrs_hmm_loglik_info", "gbrs_interpolate", "gbrs_genoprob_dosage",
    "gbrs_ri_transition_tables", "gbrs_alignment_spec",
    "gbrs_scan_create", "gbrs_scan_destroy", "gbrs_scan_append", "gbrs_scan_append_hmm", "gbrs_scan_prepare", "gbrs_scan_run",
    "gbrs_scan_info", "gbrs_scan_permute", "gbrs_scan_perm_info",
    "gbrs_scan_set_snps", "gbrs_scan_snp_dosage", "gbrs_scan_snps", "gbrs_scan_snp_info",
    "gbrs_scan_mediate", "gbrs_scan_mediate_info",
    "gbrs_scan_effects", "gbrs_scan_effects_info", "gbrs_scan_run_support",
    "gbrs_scan_kinship", "gbrs_scan_lmm_prepare", "gbrs_scan_lmm_run", "gbrs_scan_lmm_ranks", "gbrs_scan_lmm_info",
    "gbrs_scan_lmm_snps", "gbrs_scan_lmm_snp_info",
    "gbrs_scan_lmm_effects", "gbrs_scan_lmm_effects_info", "gbrs_scan_lmm_run_support",
    "gbrs_scan_int_prepare", "gbrs_scan_int_run", "gbrs_scan_int_info",
    "gbrs_compress_create", "gbrs_compress_get", "gbrs_compress_destroy",
    "gbrs_bam_open", "gbrs_bam_references", "gbrs_bam_set_reference_map", "gbrs_bam_convert", "gbrs_bam_get",
    "gbrs_bam_scan_records", "gbrs_bam_destroy",
    "gbrs_ecset_create", "gbrs_ecset_add_bam", "gbrs_ecset_add_bam_pair", "gbrs_ecset_sizes", "gbrs_ecset_get", "gbrs_ecset_destroy",
    "gbrs_matops_create", "gbrs_matops_intersect", "gbrs_matops_append_rows", "gbrs_matops_keep_unique_rows",
    "gbrs_matops_mask_columns", "gbrs_matops_sizes", "gbrs_matops_get", "gbrs_matops_destroy",
    "gbrs_matops_shared_counts", "gbrs_matops_shared_counts_get", "gbrs_matops_shared_counts_info",
    "gbrs_tensor_create", "gbrs_tensor_set_groups", "gbrs_tensor_reset", "gbrs_tensor_multiply",
    "gbrs_tensor_multiply_tensor", "gbrs_tensor_normalize", "gbrs_tensor_sum_reads", "gbrs_tensor_sum_loci",
    "gbrs_tensor_copy", "gbrs_tensor_values", "gbrs_tensor_set_values", "gbrs_tensor_nnz", "gbrs_tensor_destroy",
    "gbrs_format_double", "gbrs_write_locus_table", "gbrs_parse_length_table", "gbrs_parse_genotype_table",
    "gbrs_decode_chunks", "gbrs_inflate_backend", "gbrs_zip_directory", "gbrs_npz_stack", "gbrs_zip_read_members", "gbrs_parse_number_table",
]

GBRS_OK = 0
GBRS_ERR_INVALID = -1
GBRS_ERR_HIP = -2
GBRS_ERR_NO_DEVICE = -3
GBRS_ERR_FLOAT = -4
GBRS_ERR_UNSUPPORTED = -5
GBRS_ERR_STATE = -6

GBRS_EM_DEFAULT = 0
GBRS_EM_MERGE_IDENTICAL_ROWS = 1
GBRS_EM_LAYOUT_CSC = 2
GBRS_EM_NO_INTERLEAVE = 4
GBRS_EM_FORCE_INTERLEAVE = 8
GBRS_EM_NO_STREAMS = 16
GBRS_EM_DETERMINISTIC = 32
GBRS_EM_KEEP_CSC = 64
GBRS_EM_SIDE_BY_SIDE = 128
GBRS_EM_ONE_SHOT = 256
GBRS_EM_NO_LOCUS_SETS = 512
GBRS_EM_GROUPED_MODELS = 1024
GBRS_EM_POSTERIOR = 2048
GBRS_EM_RESAMPLE = 4096
GBRS_EM_NO_RUN_WORDS = 8192
GBRS_RESAMPLE_BASE = 0xFFFFFFFF


class EmInfo(C.Structure):
    _fields_ = [
        ("num_rows", C.c_uint64), ("num_entries", C.c_uint64), ("num_device_rows", C.c_uint64),
        ("num_device_words", C.c_uint64), ("bytes_per_iter", C.c_uint64),
        ("algorithmic_bytes", C.c_uint64), ("last_estep_ms", C.c_double),
        ("last_step_ms", C.c_double), ("num_loci", C.c_uint32), ("num_haps", C.c_uint32),
        ("layout", C.c_uint32), ("num_folded_rows", C.c_uint32),
        ("num_tiles", C.c_uint64), ("num_slots", C.c_uint64), ("num_long_rows", C.c_uint64),
        ("num_heavy_loci", C.c_uint64), ("num_light_loci", C.c_uint64), ("estep_bytes", C.c_uint64),
        ("retained_build_bytes", C.c_uint64),
        ("num_locus_sets", C.c_uint64),
    ]


class HmmInfo(C.Structure):
    _fields_ = [
        ("total_genes", C.c_uint64), ("algorithmic_bytes", C.c_uint64),
        ("last_emission_ms", C.c_double), ("last_forward_ms", C.c_double),
        ("last_backward_ms", C.c_double), ("last_backtrace_ms", C.c_double),
        ("num_states", C.c_int32), ("n_samples", C.c_int32),
        ("last_run_ms", C.c_double),
        ("last_delta_blocks", C.c_int32), ("last_delta_longest_fixup", C.c_int32),
        ("last_delta_fallbacks", C.c_int32), ("last_delta_tie_fallbacks", C.c_int32),
    ]


class ScanInfo(C.Structure):
    _fields_ = [
        ("n", C.c_int64), ("M", C.c_int64), ("H", C.c_int32), ("c", C.c_int32),
        ("last_prepare_ms", C.c_double), ("last_run_ms", C.c_double), ("last_product_ms", C.c_double),
        ("device_bytes", C.c_uint64),
    ]


class ScanPermInfo(C.Structure):
    _fields_ = [
        ("P", C.c_int64), ("B", C.c_int64), ("last_permute_ms", C.c_double), ("last_product_ms", C.c_double),
        ("peak_device_bytes", C.c_uint64),
    ]


class ScanSnpInfo(C.Structure):
    _fields_ = [
        ("M_snp", C.c_int64), ("chunk", C.c_int64), ("P", C.c_int64), ("last_pass_ms", C.c_double),
        ("last_row_ms", C.c_double), ("last_product_ms", C.c_double), ("device_bytes", C.c_uint64),
        ("peak_device_bytes", C.c_uint64), ("staged", C.c_int32), ("reserved", C.c_int32),
    ]


class ScanMediateInfo(C.Structure):
    _fields_ = [
        ("T", C.c_int64), ("Q", C.c_int64), ("last_pass_ms", C.c_double), ("last_product_ms", C.c_double),
        ("peak_device_bytes", C.c_uint64),
    ]


class ScanEffectsInfo(C.Structure):
    _fields_ = [
        ("T", C.c_int64), ("P", C.c_int64), ("last_pass_ms", C.c_double), ("peak_device_bytes", C.c_uint64),
    ]


class ScanLmmInfo(C.Structure):
    _fields_ = [
        ("cz", C.c_int32), ("n_eig", C.c_int32), ("P", C.c_int64), ("last_kinship_ms", C.c_double),
        ("last_rotate_ms", C.c_double), ("last_null_ms", C.c_double), ("last_point_ms", C.c_double),
        ("last_run_ms", C.c_double), ("device_bytes", C.c_uint64), ("peak_device_bytes", C.c_uint64),
    ]


class ScanLmmSnpInfo(C.Structure):
    _fields_ = [
        ("M_snp", C.c_int64), ("chunk", C.c_int64), ("P", C.c_int64), ("last_pass_ms", C.c_double),
        ("last_null_ms", C.c_double), ("last_rotate_ms", C.c_double), ("last_product_ms", C.c_double),
        ("column_bytes", C.c_uint64), ("peak_device_bytes", C.c_uint64),
    ]


class ScanLmmEffectsInfo(C.Structure):
    _fields_ = [
        ("T", C.c_int64), ("P", C.c_int64), ("columns", C.c_int64), ("last_pass_ms", C.c_double),
        ("last_null_ms", C.c_double), ("last_target_ms", C.c_double), ("peak_device_bytes", C.c_uint64),
    ]


class ScanIntInfo(C.Structure):
    _fields_ = [
        ("n", C.c_int64), ("M", C.c_int64), ("H", C.c_int32), ("c", C.c_int32), ("k", C.c_int32), ("HPI", C.c_int32),
        ("last_prepare_ms", C.c_double), ("last_run_ms", C.c_double), ("last_product_ms", C.c_double),
        ("device_bytes", C.c_uint64),
    ]


class GbrsHipError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(message)
        self.status = status


_lib = None


def load():
    """Load libgbrs_hip.so (once).  Raises ImportError with build instructions if missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP library has not been built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'`). "
            "gbrs_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    vp, i32, u32, u64, i64, dbl = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.c_int64, C.c_double
    pp = C.POINTER(C.c_void_p)
    lib.gbrs_last_error.restype = C.c_char_p
    lib.gbrs_last_error.argtypes = []
    lib.gbrs_abi_version.restype = i32
    lib.gbrs_device_count.restype = i32
    lib.gbrs_warm_up.restype = i32
    lib.gbrs_warm_up.argtypes = [i32]
    sigs = {
        "gbrs_em_create": [u64, u32, u32, pp, pp, vp, vp, i32, u32, pp],
        "gbrs_em_create_device": [u64, u32, u32, pp, pp, vp, vp, i32, u32, pp],
        "gbrs_em_create_masked": [u64, u32, u32, pp, pp, vp, vp, vp, i32, u32, pp],
        "gbrs_em_create_masked_device": [u64, u32, u32, pp, pp, vp, vp, vp, i32, u32, pp],
        "gbrs_em_set_initial_values": [vp, pp],
        "gbrs_em_prepare": [vp, dbl],
        "gbrs_em_step": [vp, i32, C.POINTER(dbl)],
        "gbrs_em_run": [vp, i32, dbl, i32, C.POINTER(i32), vp, i32, vp],
        "gbrs_em_set_groups": [vp, i64, vp, vp],
        "gbrs_em_step_model": [vp, i32, i32, C.POINTER(dbl)],
        "gbrs_em_posterior": [vp, u32, vp, u64],
        "gbrs_em_resample": [vp, u64, u32],
        "gbrs_em_weights": [vp, vp],
        "gbrs_em_resample_info": [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u32)],
        "gbrs_em_bootstrap_begin": [vp, i64, vp, vp],
        "gbrs_em_bootstrap_add": [vp, vp, vp, vp, vp],
        "gbrs_em_bootstrap_get": [vp, i32, C.POINTER(u32), vp, vp, vp, vp, vp, vp, vp, vp],
        "gbrs_em_get": [vp, vp, vp],
        "gbrs_em_set_theta": [vp, vp],
        "gbrs_em_group_sums": [vp, i64, vp, vp, i32, vp],
        "gbrs_em_estep_partial": [vp, pp, C.POINTER(u64)],
        "gbrs_em_finish_step": [vp, C.POINTER(dbl)],
        "gbrs_em_prepare_partial": [vp, pp, C.POINTER(u64)],
        "gbrs_em_finish_prepare": [vp, dbl],
        "gbrs_em_sync": [vp],
        "gbrs_em_pair_begin": [vp, vp, i32],
        "gbrs_em_pair_check": [vp, vp, dbl],
        "gbrs_em_pair_status": [vp, vp, C.POINTER(i32), C.POINTER(i32), vp, i32],
        "gbrs_em_set_stream": [vp, vp],
        "gbrs_em_info": [vp, C.POINTER(EmInfo)],
        "gbrs_em_fold_counts": [vp, C.POINTER(u64), C.POINTER(u64)],
        "gbrs_em_tile_cut": [vp, C.POINTER(u32), C.POINTER(u32)],
        "gbrs_em_gather_mstep": [vp, C.POINTER(u32)],
        "gbrs_em_tile_shapes": [vp, vp, vp, u64],
        "gbrs_em_stripe_census": [vp, u32, vp],
        "gbrs_alignment_counts": [u64, u32, u32, pp, pp, vp, vp, u32, i32, vp, vp, vp],
        "gbrs_counts_create": [u64, u32, u32, pp, pp, vp, i32, pp],
        "gbrs_counts_get": [vp, vp, u32, vp, vp, vp],
        "gbrs_counts_destroy": [vp],
        "gbrs_em_destroy": [vp],
        "gbrs_shard_plan": [u64, u32, u32, pp, pp, i32, i32, vp],
        "gbrs_shard_index": [u64, u32, u32, pp, pp, u64, u64, i32, pp, vp],
        "gbrs_shard_gather": [u64, u32, u32, pp, pp, u64, u64, u32, pp, i32, vp, pp, pp, C.POINTER(u64)],
        "gbrs_hmm_create": [i32, i32, vp, vp, pp, i32, pp],
        "gbrs_hmm_set_expression": [vp, i32, pp, pp, pp, dbl, dbl],
        "gbrs_hmm_set_eprob": [vp, i32, pp],
        "gbrs_hmm_run": [vp],
        "gbrs_hmm_get": [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp],
        "gbrs_hmm_info": [vp, C.POINTER(HmmInfo)],
        "gbrs_hmm_destroy": [vp],
        "gbrs_grid_knots": [i32, vp, i32, vp, vp, vp],
        "gbrs_hmm_set_grid": [vp, vp, pp, vp, pp],
        "gbrs_hmm_grid": [vp, i32, vp, vp],
        "gbrs_hmm_grid_info": [vp, C.POINTER(i64), C.POINTER(dbl)],
        "gbrs_hmm_set_panel": [vp, i32, pp],
        "gbrs_hmm_match": [vp, i32, vp, vp],
        "gbrs_hmm_match_info": [vp, C.POINTER(i32), vp, C.POINTER(dbl), C.POINTER(u64)],
        "gbrs_hmm_set_snps": [vp, vp, pp, vp, pp, pp],
        "gbrs_hmm_impute": [vp, i32, i64, i64, vp],
        "gbrs_hmm_impute_info": [vp, C.POINTER(i64), C.POINTER(dbl), C.POINTER(u64)],
        "gbrs_hmm_impute_times": [vp, C.POINTER(dbl), C.POINTER(dbl), C.POINTER(dbl)],
        "gbrs_hmm_sample_paths": [vp, i32, i32, u64, vp, vp, vp, C.POINTER(u64)],
        "gbrs_hmm_sample_info": [vp, C.POINTER(dbl), C.POINTER(u64)],
        "gbrs_hmm_diagnostics": [vp, i32, vp, vp, vp, vp, vp],
        "gbrs_hmm_pair_posterior": [vp, i32, i32, vp],
        "gbrs_hmm_diagnostics_info": [vp, C.POINTER(dbl)],
        "gbrs_hmm_loglik": [vp, i32, vp],
        "gbrs_hmm_loglik_tables": [vp, i32, i32, vp, pp, i32, vp],
        "gbrs_hmm_loglik_info": [vp, C.POINTER(dbl), C.POINTER(u64)],
        "gbrs_interpolate": [i32, i32, vp, vp, i32, vp, vp, i32],
        "gbrs_genoprob_dosage": [i32, i64, vp, vp, i32],
        "gbrs_ri_transition_tables": [vp, vp, vp, i64, dbl, dbl, i32, vp],
        "gbrs_alignment_spec": [vp, vp, vp, i64, i32, dbl, i32, vp, vp, vp, vp],
        "gbrs_scan_create": [i32, i32, vp, i32, pp],
        "gbrs_scan_destroy": [vp],
        "gbrs_scan_append": [vp, i32, vp],
        "gbrs_scan_append_hmm": [vp, vp, i32],
        "gbrs_scan_prepare": [vp, i32, vp],
        "gbrs_scan_run": [vp, i64, vp, vp, vp, vp],
        "gbrs_scan_info": [vp, C.POINTER(ScanInfo), vp],
        "gbrs_scan_permute": [vp, i64, vp, i64, u64, vp, vp, vp],
        "gbrs_scan_perm_info": [vp, C.POINTER(ScanPermInfo)],
        "gbrs_scan_set_snps": [vp, pp, vp, pp, pp],
        "gbrs_scan_snp_dosage": [vp, i64, i64, vp],
        "gbrs_scan_snps": [vp, i64, vp, vp, vp, vp, vp],
        "gbrs_scan_snp_info": [vp, C.POINTER(ScanSnpInfo)],
        "gbrs_scan_mediate": [vp, i64, vp, vp, i64, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp],
        "gbrs_scan_mediate_info": [vp, C.POINTER(ScanMediateInfo)],
        "gbrs_scan_effects": [vp, i64, vp, i64, vp, vp, vp, vp, vp, vp, vp],
        "gbrs_scan_effects_info": [vp, C.POINTER(ScanEffectsInfo)],
        "gbrs_scan_run_support": [vp, i64, vp, dbl, vp, vp, vp, vp, vp],
        "gbrs_scan_kinship": [vp, i32, dbl, vp],
        "gbrs_scan_lmm_prepare": [vp, i32, vp, i32, pp, pp, vp],
        "gbrs_scan_lmm_run": [vp, i64, vp, vp, vp, vp, vp, vp, vp],
        "gbrs_scan_lmm_ranks": [vp, vp, vp],
        "gbrs_scan_lmm_info": [vp, C.POINTER(ScanLmmInfo)],
        "gbrs_scan_lmm_snps": [vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp],
        "gbrs_scan_lmm_snp_info": [vp, C.POINTER(ScanLmmSnpInfo)],
        "gbrs_scan_lmm_effects": [vp, i64, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp],
        "gbrs_scan_lmm_effects_info": [vp, C.POINTER(ScanLmmEffectsInfo)],
        "gbrs_scan_lmm_run_support": [vp, i64, vp, vp, C.c_double, vp, vp, vp, vp, vp, vp, vp],
        "gbrs_scan_int_prepare": [vp, i32, vp, i32, vp],
        "gbrs_scan_int_run": [vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp],
        "gbrs_scan_int_info": [vp, C.POINTER(ScanIntInfo), vp, vp],
        "gbrs_compress_create": [u64, u32, u32, pp, pp, vp, i32, pp, C.POINTER(u64), vp],
        "gbrs_compress_get": [vp, pp, pp, vp],
        "gbrs_compress_destroy": [vp],
        "gbrs_bam_convert": [vp, i32, C.POINTER(u64), C.POINTER(u32), vp, vp],
        "gbrs_bam_get": [vp, pp, pp, vp],
        "gbrs_ecset_create": [u32, u32, i32, C.POINTER(vp)],
        "gbrs_ecset_add_bam": [vp, vp, C.POINTER(u64), vp],
        "gbrs_ecset_add_bam_pair": [vp, vp, vp, C.POINTER(u64), vp],
        "gbrs_ecset_sizes": [vp, C.POINTER(u64), C.POINTER(u64), vp],
        "gbrs_ecset_get": [vp, pp, pp, vp],
        "gbrs_ecset_destroy": [vp],
        "gbrs_matops_create": [u64, u32, u32, pp, pp, i32, pp],
        "gbrs_matops_intersect": [vp, pp, pp],
        "gbrs_matops_append_rows": [vp, u64, pp, pp],
        "gbrs_matops_keep_unique_rows": [vp, vp, u32, i32, vp],
        "gbrs_matops_mask_columns": [vp, vp],
        "gbrs_matops_sizes": [vp, C.POINTER(u64), vp, C.POINTER(u32)],
        "gbrs_matops_get": [vp, pp, pp],
        "gbrs_matops_destroy": [vp],
        "gbrs_matops_shared_counts": [vp, vp, u32, C.POINTER(u64)],
        "gbrs_matops_shared_counts_get": [vp, vp, vp, vp],
        "gbrs_matops_shared_counts_info": [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), C.POINTER(u32),
                                           C.POINTER(u64), C.POINTER(u64), C.POINTER(dbl)],
        "gbrs_tensor_create": [u64, u32, u32, pp, pp, pp, vp, i32, pp],
        "gbrs_tensor_set_groups": [vp, i64, vp, vp],
        "gbrs_tensor_reset": [vp],
        "gbrs_tensor_multiply": [vp, i32, vp, u64],
        "gbrs_tensor_multiply_tensor": [vp, vp],
        "gbrs_tensor_normalize": [vp, i32],
        "gbrs_tensor_sum_reads": [vp, vp],
        "gbrs_tensor_sum_loci": [vp, vp],
        "gbrs_tensor_copy": [vp, pp],
        "gbrs_tensor_values": [vp, u32, vp, vp, u64],
        "gbrs_tensor_set_values": [vp, u32, vp, u64],
        "gbrs_tensor_nnz": [vp, vp],
        "gbrs_tensor_destroy": [vp],
    }
    sigs.update(_host_signatures())
    for name, args in sigs.items():
        if name in ("gbrs_em_fold_counts", "gbrs_em_tile_cut", "gbrs_em_gather_mstep", "gbrs_em_tile_shapes", "gbrs_em_stripe_census") and os.environ.get("GBRS_TUNING_LIB") and not hasattr(lib, name):
            continue        # an A/B variant built from a commit before the call existed
        fn = getattr(lib, name)
        fn.restype = i32
        fn.argtypes = args
    lib.gbrs_em_stream.restype = vp
    lib.gbrs_em_stream.argtypes = [vp]
    if lib.gbrs_abi_version() != 5:
        raise ImportError("libgbrs_hip.so ABI version mismatch")
    _lib = lib
    return lib


def _host_signatures():
    """The host-only entry points of the library (gbrs_amd/csrc/hostio.hip, bamio.hip)."""
    vp, i32, u32, u64, i64, dbl = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.c_int64, C.c_double
    return {
        "gbrs_format_double": [dbl, C.c_char_p],
        "gbrs_decode_chunks": [C.c_char_p, i64, vp, vp, vp, vp, u64, u32, u64, i32, i32, vp, i32],
        "gbrs_inflate_backend": [],
        "gbrs_zip_directory": [vp, u64, u64, vp, vp, vp, vp, vp, vp, u64, C.POINTER(u64), C.POINTER(u64)],
        "gbrs_npz_stack": [vp, u64, i64, vp, vp, vp, vp, vp, vp, u64, u64, vp, vp, i32],
        "gbrs_zip_read_members": [vp, u64, i64, vp, vp, vp, vp, vp, vp, i32],
        "gbrs_parse_number_table": [C.c_char_p, i64, i64, i32, vp],
        "gbrs_parse_length_table": [C.c_char_p, i64, C.c_char_p, vp, i64, C.c_char_p, vp, i32, dbl, vp],
        "gbrs_parse_genotype_table": [C.c_char_p, i64, C.c_char_p, vp, i64, C.c_char_p, vp, i32, vp, vp, i32, vp,
                                      C.POINTER(i64)],
        "gbrs_bam_open": [C.c_char_p, i32, C.POINTER(vp), C.POINTER(u64), C.POINTER(u64)],
        "gbrs_bam_references": [vp, vp, u64, vp, vp],
        "gbrs_bam_set_reference_map": [vp, u64, vp, vp, u32, u32],
        "gbrs_bam_scan_records": [vp, u64, vp, vp, vp, vp, u64, C.POINTER(u64), C.POINTER(u64)],
        "gbrs_bam_destroy": [vp],
        "gbrs_write_locus_table": [C.c_char_p, C.c_char_p, vp, i64, i32, i64, i64, vp, C.c_char_p, vp, C.c_char_p, vp, vp],
    }


def check(status):
    """Map a gbrs_status to the exception the reference would have raised."""
    if status == GBRS_OK:
        return
    msg = load().gbrs_last_error().decode(errors="replace")
    if status == GBRS_ERR_FLOAT:
        raise FloatingPointError(msg)
    raise GbrsHipError(status, msg)


def ptr(a):
    """void* of a C-contiguous numpy array (or None)."""
    if a is None:
        return None
    return a.ctypes.data_as(C.c_void_p)


def ptr_table(arrays):
    """host array of H pointers to the given numpy arrays (kept alive by the caller)."""
    tab = (C.c_void_p * len(arrays))()
    for i, a in enumerate(arrays):
        tab[i] = None if a is None else a.ctypes.data
    return tab


def raw_table(addresses):
    tab = (C.c_void_p * len(addresses))()
    for i, a in enumerate(addresses):
        tab[i] = a
    return tab


def warm_up_device_async(device=0):
    """Start the HIP runtime (library load, hipInit, device context: ~0.15-0.3 s in a fresh process) on a
    background thread so that it overlaps with reading the input files; ctypes releases the GIL during
    the call.  Returns the thread (join() is optional: the first real call blocks on the runtime's own
    initialisation lock anyway)."""
    import threading

    def _go():
        try:
            load().gbrs_warm_up(int(device))
        except Exception:      # noqa: BLE001 - the foreground call will report the problem
            pass
    t = threading.Thread(target=_go, name='gbrs-hip-init', daemon=True)
    t.start()
    return t
