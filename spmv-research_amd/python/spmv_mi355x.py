"""ctypes binding of the C ABI in include/spmv_mi355x.h (libspmv_mi355x.so, hand-written HIP for gfx950).

This is test/bench plumbing above the C ABI: the same entry points the reference harness would bind through
host/spmv_kernel_mi355x.cpp. There is no fallback: if the shared object is missing or no GPU is usable, the
calls raise.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(_HERE)
LIB_PATH = os.environ.get("SPMV_MI355X_LIB") or os.path.join(PKG_ROOT, "lib", "libspmv_mi355x.so")     # the override is for kernel experiments

CSR_SCALAR, CSR_VECTOR, CSR_MERGE, SELL_C_SIGMA, COO, CSR_STREAM = range(6)
FORMATS = {"csr_scalar": CSR_SCALAR, "csr_vector": CSR_VECTOR, "csr_merge": CSR_MERGE,
           "sell_c_sigma": SELL_C_SIGMA, "coo": COO, "csr_stream": CSR_STREAM}
F64, F32 = 0, 1


class Opts(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("device", C.c_int), ("lanes_per_row", C.c_int),
                ("sell_split", C.c_int), ("sell_c", C.c_int), ("sell_sigma", C.c_int),
                ("merge_items", C.c_int), ("xcd_remap", C.c_int), ("nontemporal", C.c_int),
                ("stream_mode", C.c_int),
                ("row_begin", C.c_long), ("row_end", C.c_long), ("col_begin", C.c_long), ("col_end", C.c_long),
                ("col_filter_mode", C.c_int), ("sell_delta", C.c_int), ("convert_on", C.c_int),
                ("symmetric_input", C.c_int), ("rows_per_group", C.c_int), ("col_blocks", C.c_int),
                ("sell_window", C.c_int), ("kahan", C.c_int), ("sell_group", C.c_int), ("placement", C.c_int),
                ("placement_budget_gib", C.c_int), ("sell_values", C.c_int), ("value_storage", C.c_int)]


# opts.transpose, the last field of spmv_mi355x_opts (include/spmv_mi355x.h "transposed handles"). In C it took the struct's tail
# padding: sizeof did not change, and the field sits right behind value_storage, inside what ctypes counts as padding of the
# _fields_ above. That list is pinned by the ABI tests of the options before it, so the mirror of this field is a property over the
# same bytes: Opts().transpose reads and writes the int at OPTS_TRANSPOSE_OFFSET.
OPTS_TRANSPOSE_OFFSET = Opts.value_storage.offset + C.sizeof(C.c_int)
assert OPTS_TRANSPOSE_OFFSET + C.sizeof(C.c_int) <= C.sizeof(Opts), "spmv_mi355x_opts has no room behind value_storage"
Opts.transpose = property(lambda self: C.c_int.from_buffer(self, OPTS_TRANSPOSE_OFFSET).value,
                          lambda self, v: setattr(C.c_int.from_buffer(self, OPTS_TRANSPOSE_OFFSET), "value", v))


# every symbol declared in include/spmv_mi355x.h (checked by tests/test_abi.py)
SYMBOLS = [
    "spmv_mi355x_last_error", "spmv_mi355x_device_count", "spmv_mi355x_device_info", "spmv_mi355x_create",
    "spmv_mi355x_destroy", "spmv_mi355x_format_name", "spmv_mi355x_mem_footprint", "spmv_mi355x_csr_mem_footprint",
    "spmv_mi355x_rows", "spmv_mi355x_cols", "spmv_mi355x_nnz", "spmv_mi355x_spmv", "spmv_mi355x_set_always_copy",
    "spmv_mi355x_upload_x", "spmv_mi355x_download_y", "spmv_mi355x_spmv_device_async", "spmv_mi355x_time_device",
    "spmv_mi355x_kernel_info", "spmv_mi355x_x_device", "spmv_mi355x_y_device", "spmv_mi355x_sell_layout", "spmv_mi355x_stored_array",
    "spmv_mi355x_merge_tiles", "spmv_mi355x_free", "spmv_mi355x_precision", "spmv_mi355x_value_storage", "spmv_mi355x_device",
    "spmv_mi355x_transposed",
    "spmv_mi355x_pcg", "spmv_mi355x_pbicgstab", "spmv_mi355x_pcg_dist", "spmv_mi355x_pbicgstab_dist",
    "spmv_mi355x_pcg_multi", "spmv_mi355x_pbicgstab_multi", "spmv_mi355x_cgls", "spmv_mi355x_minres", "spmv_mi355x_gmres",
    "spmv_mi355x_copy_device_async",
    "spmv_mi355x_create_partitioned", "spmv_mi355x_destroy_partitioned", "spmv_mi355x_spmv_partitioned",
    "spmv_mi355x_partitioned_set_always_copy", "spmv_mi355x_time_partitioned", "spmv_mi355x_partitioned_parts",
    "spmv_mi355x_partitioned_offsets", "spmv_mi355x_partitioned_format_name", "spmv_mi355x_partitioned_exchange",
    "spmv_mi355x_partitioned_mem_footprint",
    "spmv_mi355x_upload_y", "spmv_mi355x_output_alloc", "spmv_mi355x_input_alloc", "spmv_mi355x_output_free", "spmv_mi355x_placement_release", "spmv_mi355x_placement_info", "spmv_mi355x_place_arrays",
    "spmv_mi355x_csr_stream_begin", "spmv_mi355x_csr_stream_append", "spmv_mi355x_create_from_stream", "spmv_mi355x_csr_stream_discard",
    "spmv_mi355x_spmm_device_async", "spmv_mi355x_time_spmm_device", "spmv_mi355x_spmm", "spmv_mi355x_spmm_plan",
    "spmv_mi355x_update_values_prepare", "spmv_mi355x_update_values", "spmv_mi355x_update_values_device", "spmv_mi355x_update_values_state",
    "spmv_mi355x_update_values_prepare_transposed", "spmv_mi355x_update_values_count",
    "spmv_mi355x_trsv_analyze", "spmv_mi355x_trsv_create", "spmv_mi355x_trsv_destroy", "spmv_mi355x_trsv_solve_device_async",
    "spmv_mi355x_trsv_solve", "spmv_mi355x_trsv_info", "spmv_mi355x_trsv_mem_footprint", "spmv_mi355x_time_trsv_device",
    "spmv_mi355x_trsv_analyze_blocked", "spmv_mi355x_trsv_create_blocked", "spmv_mi355x_trsv_block_info", "spmv_mi355x_gmres_tri",
    "spmv_mi355x_pcg_tri",
    "spmv_mi355x_fsai_pattern", "spmv_mi355x_fsai_create", "spmv_mi355x_fsai_destroy", "spmv_mi355x_fsai_apply_device_async",
    "spmv_mi355x_fsai_apply", "spmv_mi355x_fsai_values", "spmv_mi355x_fsai_matrices", "spmv_mi355x_fsai_info",
    "spmv_mi355x_fsai_setup_split", "spmv_mi355x_fsai_mem_footprint", "spmv_mi355x_pcg_fsai",
    "spmv_mi355x_spgemm_create", "spmv_mi355x_spgemm_destroy", "spmv_mi355x_spgemm_pattern", "spmv_mi355x_spgemm_multiply",
    "spmv_mi355x_spgemm_multiply_device_async", "spmv_mi355x_spgemm_info",
    "spmv_mi355x_amg_create", "spmv_mi355x_amg_destroy", "spmv_mi355x_amg_apply_device_async", "spmv_mi355x_amg_apply",
    "spmv_mi355x_amg_info", "spmv_mi355x_amg_level_matrices", "spmv_mi355x_amg_aggregates", "spmv_mi355x_amg_level_csr",
    "spmv_mi355x_amg_mem_footprint", "spmv_mi355x_pcg_amg",
    "spmv_mi355x_amg_update_values_prepare", "spmv_mi355x_amg_update_values", "spmv_mi355x_amg_update_values_device",
    "spmv_mi355x_amg_update_values_state", "spmv_mi355x_amg_update_info",
    "spmv_mi355x_amg_create_with", "spmv_mi355x_amg_prolongator_info", "spmv_mi355x_amg_near_null",
    "spmv_mi355x_amg_apply_multi_device_async", "spmv_mi355x_amg_apply_multi", "spmv_mi355x_amg_apply_multi_plan",
    "spmv_mi355x_amg_set_fold", "spmv_mi355x_amg_fold_info", "spmv_mi355x_amg_apply_level_device_async",
    "spmv_mi355x_fsai_apply_multi_device_async", "spmv_mi355x_fsai_apply_multi",
    "spmv_mi355x_pcg_tri_multi", "spmv_mi355x_pcg_fsai_multi", "spmv_mi355x_pcg_amg_multi",
    "spmv_mi355x_trsv_solve_multi_device_async", "spmv_mi355x_trsv_solve_multi", "spmv_mi355x_trsv_solve_multi_plan",
    "spmv_mi355x_time_trsv_multi_device", "spmv_mi355x_pcg_trsm_multi",
    "spmv_mi355x_ilu0_create", "spmv_mi355x_ilu0_factor", "spmv_mi355x_ilu0_factor_device_async", "spmv_mi355x_ilu0_values",
    "spmv_mi355x_ilu0_values_device", "spmv_mi355x_ilu0_get_info", "spmv_mi355x_ilu0_mem_footprint", "spmv_mi355x_ilu0_destroy",
    "spmv_mi355x_trsv_update_map", "spmv_mi355x_trsv_update_values_prepare", "spmv_mi355x_trsv_update_values_bytes",
    "spmv_mi355x_trsv_update_values_state", "spmv_mi355x_trsv_update_values_device_async", "spmv_mi355x_trsv_update_values_result",
    "spmv_mi355x_trsv_update_values_device", "spmv_mi355x_trsv_update_values", "spmv_mi355x_trsv_stored_values",
    "spmv_mi355x_trsv_update_values_staged",
    "spmv_mi355x_trsv_solve_sweeps_device_async", "spmv_mi355x_trsv_solve_sweeps", "spmv_mi355x_trsv_solve_sweeps_multi_device_async",
    "spmv_mi355x_trsv_solve_sweeps_multi", "spmv_mi355x_trsv_set_sweeps", "spmv_mi355x_trsv_sweeps_info",
    "spmv_mi355x_color_create", "spmv_mi355x_color_destroy", "spmv_mi355x_color_info", "spmv_mi355x_color_colors", "spmv_mi355x_color_perm",
    "spmv_mi355x_color_color_ptr", "spmv_mi355x_color_mem_footprint", "spmv_mi355x_color_permute_csr", "spmv_mi355x_color_permute_csr_device",
    "spmv_mi355x_color_permute_values", "spmv_mi355x_color_permute_values_device_async", "spmv_mi355x_color_permute_vectors",
    "spmv_mi355x_color_permute_vectors_device_async",
]

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `make -C spmv-research_amd` "
                               "(__graft_entry__.build()). There is no CPU fallback.")
        # One HIP runtime per process: torch bundles its own libamdhip64.so.7 and refuses to initialise ("No HIP GPUs
        # are available") when the system copy was loaded first. Loading torch's first lets both share it.
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        L = C.CDLL(LIB_PATH)
        L.spmv_mi355x_last_error.restype = C.c_char_p
        L.spmv_mi355x_format_name.restype = C.c_char_p
        L.spmv_mi355x_mem_footprint.restype = C.c_double
        L.spmv_mi355x_csr_mem_footprint.restype = C.c_double
        for f in ("spmv_mi355x_rows", "spmv_mi355x_cols", "spmv_mi355x_nnz", "spmv_mi355x_update_values_count"):
            getattr(L, f).restype = C.c_long
        L.spmv_mi355x_partitioned_format_name.restype = C.c_char_p
        L.spmv_mi355x_partitioned_exchange.restype = C.c_char_p
        L.spmv_mi355x_partitioned_mem_footprint.restype = C.c_double
        L.spmv_mi355x_trsv_mem_footprint.restype = C.c_double
        L.spmv_mi355x_x_device.restype = C.c_void_p
        L.spmv_mi355x_y_device.restype = C.c_void_p
        L.spmv_mi355x_cgls.restype = C.c_int
        L.spmv_mi355x_cgls.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_long,
                                       C.c_void_p, C.POINTER(LsqInfo)]
        L.spmv_mi355x_minres.restype = C.c_int
        L.spmv_mi355x_minres.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_double, C.c_long,
                                         C.c_void_p, C.POINTER(MinresInfo)]
        L.spmv_mi355x_gmres.restype = C.c_int
        L.spmv_mi355x_gmres.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_long,
                                        C.c_void_p, C.POINTER(GmresInfo)]
        L.spmv_mi355x_gmres_tri.restype = C.c_int
        L.spmv_mi355x_gmres_tri.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(TriPrecond), C.c_double, C.c_long,
                                            C.c_void_p, C.POINTER(GmresInfo)]
        L.spmv_mi355x_pcg_tri.restype = C.c_int
        L.spmv_mi355x_pcg_tri.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(TriPrecond), C.c_double, C.c_long,
                                          C.c_void_p, C.POINTER(PcgTriInfo)]
        L.spmv_mi355x_pcg_fsai.restype = C.c_int
        L.spmv_mi355x_pcg_fsai.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_long, C.c_void_p,
                                           C.POINTER(PcgTriInfo)]
        L.spmv_mi355x_fsai_mem_footprint.restype = C.c_double
        L.spmv_mi355x_pcg_amg.restype = C.c_int
        L.spmv_mi355x_pcg_amg.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_long, C.c_void_p,
                                          C.POINTER(PcgTriInfo)]
        L.spmv_mi355x_amg_mem_footprint.restype = C.c_double
        for f in ("spmv_mi355x_amg_update_values_prepare", "spmv_mi355x_amg_update_values_state"):
            getattr(L, f).restype = C.c_int
            getattr(L, f).argtypes = [C.c_void_p]
        L.spmv_mi355x_amg_update_values.restype = C.c_int
        L.spmv_mi355x_amg_update_values.argtypes = [C.c_void_p, C.c_void_p]
        L.spmv_mi355x_amg_update_values_device.restype = C.c_int
        L.spmv_mi355x_amg_update_values_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.spmv_mi355x_amg_update_info.restype = C.c_int
        L.spmv_mi355x_amg_update_info.argtypes = [C.c_void_p, C.c_void_p]
        for f in ("spmv_mi355x_amg_apply_multi_device_async", "spmv_mi355x_fsai_apply_multi_device_async"):
            getattr(L, f).restype = C.c_int
            getattr(L, f).argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p]
        for f in ("spmv_mi355x_amg_apply_multi", "spmv_mi355x_fsai_apply_multi"):
            getattr(L, f).restype = C.c_int
            getattr(L, f).argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.spmv_mi355x_amg_apply_multi_plan.restype = C.c_int
        L.spmv_mi355x_amg_apply_multi_plan.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_long), C.POINTER(C.c_long)]
        L.spmv_mi355x_amg_set_fold.restype = C.c_int
        L.spmv_mi355x_amg_set_fold.argtypes = [C.c_void_p, C.c_int]
        L.spmv_mi355x_amg_fold_info.restype = C.c_int
        L.spmv_mi355x_amg_fold_info.argtypes = [C.c_void_p, C.c_void_p]
        L.spmv_mi355x_amg_apply_level_device_async.restype = C.c_int
        L.spmv_mi355x_amg_apply_level_device_async.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        for f in ("spmv_mi355x_pcg_tri_multi", "spmv_mi355x_pcg_trsm_multi"):
            getattr(L, f).restype = C.c_int
            getattr(L, f).argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(TriPrecond), C.c_double, C.c_long,
                                      C.c_void_p, C.c_void_p]
        L.spmv_mi355x_trsv_solve_multi_device_async.restype = C.c_int
        L.spmv_mi355x_trsv_solve_multi_device_async.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p]
        L.spmv_mi355x_trsv_solve_multi.restype = C.c_int
        L.spmv_mi355x_trsv_solve_multi.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.spmv_mi355x_trsv_solve_sweeps_device_async.restype = C.c_int
        L.spmv_mi355x_trsv_solve_sweeps_device_async.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.spmv_mi355x_trsv_solve_sweeps.restype = C.c_int
        L.spmv_mi355x_trsv_solve_sweeps.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.spmv_mi355x_trsv_solve_sweeps_multi_device_async.restype = C.c_int
        L.spmv_mi355x_trsv_solve_sweeps_multi_device_async.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_void_p,
                                                                       C.c_long, C.c_void_p]
        L.spmv_mi355x_trsv_solve_sweeps_multi.restype = C.c_int
        L.spmv_mi355x_trsv_solve_sweeps_multi.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.spmv_mi355x_trsv_set_sweeps.restype = C.c_int
        L.spmv_mi355x_trsv_set_sweeps.argtypes = [C.c_void_p, C.c_int]
        L.spmv_mi355x_trsv_sweeps_info.restype = C.c_int
        L.spmv_mi355x_trsv_sweeps_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_long), C.POINTER(C.c_long),
                                                   C.POINTER(C.c_double)]
        L.spmv_mi355x_trsv_solve_multi_plan.restype = C.c_int
        L.spmv_mi355x_trsv_solve_multi_plan.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_int)]
        L.spmv_mi355x_time_trsv_multi_device.restype = C.c_int
        L.spmv_mi355x_time_trsv_multi_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_int,
                                                         C.c_void_p, C.POINTER(C.c_double)]
        for f in ("spmv_mi355x_pcg_fsai_multi", "spmv_mi355x_pcg_amg_multi"):
            getattr(L, f).restype = C.c_int
            getattr(L, f).argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_long, C.c_void_p,
                                      C.c_void_p]
        L.spmv_mi355x_ilu0_create.restype = C.c_int
        L.spmv_mi355x_ilu0_create.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_long, C.c_int]
        for f in ("spmv_mi355x_ilu0_factor", "spmv_mi355x_ilu0_values", "spmv_mi355x_ilu0_values_device", "spmv_mi355x_ilu0_get_info"):
            getattr(L, f).restype = C.c_int
            getattr(L, f).argtypes = [C.c_void_p, C.c_void_p]
        L.spmv_mi355x_ilu0_factor_device_async.restype = C.c_int
        L.spmv_mi355x_ilu0_factor_device_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.spmv_mi355x_ilu0_mem_footprint.restype = C.c_double
        L.spmv_mi355x_ilu0_mem_footprint.argtypes = [C.c_void_p]
        L.spmv_mi355x_ilu0_destroy.restype = C.c_int
        L.spmv_mi355x_ilu0_destroy.argtypes = [C.c_void_p]
        L.spmv_mi355x_trsv_update_map.restype = C.c_int
        L.spmv_mi355x_trsv_update_map.argtypes = [C.c_int, C.c_int, C.c_long, C.c_void_p, C.c_void_p, C.c_int, C.c_long, C.c_void_p,
                                                  C.POINTER(C.c_long), C.c_void_p]
        L.spmv_mi355x_trsv_update_values_prepare.restype = C.c_int
        L.spmv_mi355x_trsv_update_values_prepare.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_void_p]
        L.spmv_mi355x_trsv_update_values_bytes.restype = C.c_double
        L.spmv_mi355x_trsv_update_values_bytes.argtypes = [C.c_void_p]
        L.spmv_mi355x_trsv_update_values_state.restype = C.c_int
        L.spmv_mi355x_trsv_update_values_state.argtypes = [C.c_void_p]
        for f in ("spmv_mi355x_trsv_update_values_device_async", "spmv_mi355x_trsv_update_values_device"):
            getattr(L, f).restype = C.c_int
            getattr(L, f).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.spmv_mi355x_trsv_update_values_result.restype = C.c_int
        L.spmv_mi355x_trsv_update_values_result.argtypes = [C.c_void_p, C.POINTER(C.c_long)]
        L.spmv_mi355x_trsv_update_values.restype = C.c_int
        L.spmv_mi355x_trsv_update_values.argtypes = [C.c_void_p, C.c_void_p]
        L.spmv_mi355x_trsv_update_values_staged.restype = C.c_int
        L.spmv_mi355x_trsv_update_values_staged.argtypes = [C.c_void_p, C.c_void_p]
        L.spmv_mi355x_trsv_stored_values.restype = C.c_int
        L.spmv_mi355x_trsv_stored_values.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_long), C.c_void_p]
        L.spmv_mi355x_color_create.restype = C.c_int
        L.spmv_mi355x_color_create.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_int]
        for f in ("spmv_mi355x_color_info", "spmv_mi355x_color_colors", "spmv_mi355x_color_color_ptr"):
            getattr(L, f).restype = C.c_int
            getattr(L, f).argtypes = [C.c_void_p, C.c_void_p]
        for f in ("spmv_mi355x_color_perm", "spmv_mi355x_color_permute_values"):
            getattr(L, f).restype = C.c_int
            getattr(L, f).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.spmv_mi355x_color_mem_footprint.restype = C.c_double
        L.spmv_mi355x_color_mem_footprint.argtypes = [C.c_void_p]
        L.spmv_mi355x_color_destroy.restype = C.c_int
        L.spmv_mi355x_color_destroy.argtypes = [C.c_void_p]
        L.spmv_mi355x_color_permute_csr.restype = C.c_int
        L.spmv_mi355x_color_permute_csr.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        for f in ("spmv_mi355x_color_permute_csr_device", "spmv_mi355x_color_permute_values_device_async"):
            getattr(L, f).restype = C.c_int
            getattr(L, f).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.spmv_mi355x_color_permute_vectors.restype = C.c_int
        L.spmv_mi355x_color_permute_vectors.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_long]
        L.spmv_mi355x_color_permute_vectors_device_async.restype = C.c_int
        L.spmv_mi355x_color_permute_vectors_device_async.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_void_p,
                                                                     C.c_long, C.c_void_p]
        _lib = L
    return _lib


class SpmvError(RuntimeError):
    pass


def _check(rc):
    if rc != 0:
        raise SpmvError(lib().spmv_mi355x_last_error().decode())


def placement_release(device=-1):
    """Free the vector pools of a device (-1: all) — no vector of them may be live (include/spmv_mi355x.h)."""
    _check(lib().spmv_mi355x_placement_release(C.c_int(device)))


def placement_info(device=0):
    """What the one walk of a device found (include/spmv_mi355x.h): dict(state, candidates, walked_gib, pools, us_per_pool)."""
    st, cand, gib, npool, us = C.c_int(), C.c_int(), C.c_long(), C.c_int(), (C.c_double * 4)()
    _check(lib().spmv_mi355x_placement_info(C.c_int(device), C.byref(st), C.byref(cand), C.byref(gib), C.byref(npool), us))
    return dict(state={0: "no walk", 1: "pools kept", 2: "no contrast: plain allocations"}[st.value], candidates=cand.value, walked_gib=gib.value,
                pools=npool.value, us_per_pool=[round(us[k], 1) for k in range(npool.value)])


def device_count():
    c = C.c_int()
    _check(lib().spmv_mi355x_device_count(C.byref(c)))
    return c.value


def device_info(device=0):
    name = C.create_string_buffer(256)
    cu = C.c_int()
    mem = C.c_long()
    _check(lib().spmv_mi355x_device_info(device, name, C.c_long(256), C.byref(cu), C.byref(mem)))
    return dict(name=name.value.decode(), compute_units=cu.value, hbm_bytes=mem.value)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class OutputVector:
    """A device vector a handle's SpMV writes, allocated by the engine (include/spmv_mi355x.h "output vectors placed by the
    engine"): placed by timing the handle's own kernel on it. `.ptr` goes to spmv_device(); `.torch()` is a zero-copy torch
    view (CUDA array interface) for callers that fill / check it with torch."""

    def __init__(self, matrix, count, is_input=False):
        self.count, self.dtype = int(count), np.dtype(matrix.dtype)
        self.nbytes = max(self.count, 1) * self.dtype.itemsize
        out = C.c_void_p()
        alloc = lib().spmv_mi355x_input_alloc if is_input else lib().spmv_mi355x_output_alloc
        _check(alloc(matrix.h, C.c_size_t(self.nbytes), C.byref(out)))
        self.ptr = out.value
        self._view = None

    @property
    def __cuda_array_interface__(self):
        return dict(shape=(self.count,), typestr=self.dtype.str, data=(self.ptr, False), version=2, strides=None)

    def torch(self):
        import torch
        if self._view is None:
            self._view = torch.as_tensor(self, device="cuda")
        return self._view

    def free(self):
        if getattr(self, "ptr", None):
            self._view = None
            lib().spmv_mi355x_output_free(C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _make_opts(opts):
    o = Opts()
    o.struct_size = C.sizeof(Opts)
    o.device = -1
    for k, v in opts.items():
        if not hasattr(o, k):
            raise TypeError(f"unknown option {k}")
        setattr(o, k, v)
    return o


class CsrStream:
    """A CSR assembled in device memory from pieces of consecutive rows (include/spmv_mi355x.h "a handle from a CSR that arrives in
    pieces"): append(row_ptr, col_idx, values) per piece, finish(fmt, dtype, **opts) -> Matrix. The host never holds more than a
    piece. SELL-C-sigma (64-row slices, delta layout) only. finish(..., transpose=1) gives the handle of the transposed matrix,
    transposed on the GPU from the resident arrays."""

    def __init__(self, m, n, nnz_capacity, device=-1):
        self.s = C.c_void_p()
        _check(lib().spmv_mi355x_csr_stream_begin(C.byref(self.s), C.c_int(device), C.c_long(m), C.c_long(n), C.c_long(nnz_capacity)))

    def append(self, row_ptr, col_idx, values):
        row_ptr = np.ascontiguousarray(row_ptr, np.int32)
        col_idx = np.ascontiguousarray(col_idx, np.int32)
        values = np.ascontiguousarray(values, np.float64)
        _check(lib().spmv_mi355x_csr_stream_append(self.s, C.c_long(len(row_ptr) - 1), _p(row_ptr), _p(col_idx), _p(values)))

    def finish(self, fmt="sell_c_sigma", dtype=np.float64, **opts):
        o = _make_opts(opts)
        h = C.c_void_p()
        s, self.s = self.s, None                       # consumed, whatever happens
        fmt_id = FORMATS[fmt] if isinstance(fmt, str) else fmt
        _check(lib().spmv_mi355x_create_from_stream(C.byref(h), s, fmt_id, F64 if np.dtype(dtype) == np.float64 else F32, C.byref(o)))
        return Matrix(None, None, None, 0, 0, fmt, dtype, _handle=h)

    def discard(self):
        if getattr(self, "s", None):
            lib().spmv_mi355x_csr_stream_discard(self.s)
            self.s = None

    def __del__(self):
        try:
            self.discard()
        except Exception:
            pass


LOWER, UPPER = 0, 1
DIAG_STORED, DIAG_UNIT = 0, 1
_UPLO = {"lower": LOWER, "upper": UPPER, LOWER: LOWER, UPPER: UPPER}
_DIAG = {"stored": DIAG_STORED, "unit": DIAG_UNIT, DIAG_STORED: DIAG_STORED, DIAG_UNIT: DIAG_UNIT}


def trsv_analyze(row_ptr, col_idx, n, uplo, chain_rows=0):
    """What TriangularSolve derives from the pattern, on the host (spmv_mi355x_trsv_analyze): dict(level_of_row, levels, launches,
    max_level_rows, chain_rows), chain_rows being the threshold used (the default when 0 was passed)."""
    row_ptr = np.ascontiguousarray(row_ptr, np.int32)
    col_idx = np.ascontiguousarray(col_idx, np.int32)
    lv = C.POINTER(C.c_int32)()
    levels, launches, widest, used = C.c_long(), C.c_long(), C.c_long(), C.c_int()
    _check(lib().spmv_mi355x_trsv_analyze(C.c_int(_UPLO[uplo]), C.c_long(n), _p(row_ptr), _p(col_idx), C.c_int(chain_rows), C.byref(lv),
                                          C.byref(levels), C.byref(launches), C.byref(widest), C.byref(used)))
    level_of_row = np.ctypeslib.as_array(lv, shape=(max(n, 1),))[:n].copy()
    lib().spmv_mi355x_free(lv)
    return dict(level_of_row=level_of_row, levels=levels.value, launches=launches.value, max_level_rows=widest.value,
                chain_rows=used.value)


def trsv_analyze_blocked(row_ptr, col_idx, n, uplo, block_rows=0):
    """What a blocked TriangularSolve derives from the pattern, on the host (spmv_mi355x_trsv_analyze_blocked): dict(level_of_row,
    blocks, max_block_levels, max_level_rows, nnz_dropped, block_rows), level_of_row being the level of each row within its block and
    block_rows the size used (the default when 0 was passed)."""
    row_ptr = np.ascontiguousarray(row_ptr, np.int32)
    col_idx = np.ascontiguousarray(col_idx, np.int32)
    lv = C.POINTER(C.c_int32)()
    blocks, levels, widest, dropped, used = C.c_long(), C.c_long(), C.c_long(), C.c_long(), C.c_long()
    _check(lib().spmv_mi355x_trsv_analyze_blocked(C.c_int(_UPLO[uplo]), C.c_long(n), _p(row_ptr), _p(col_idx), C.c_long(block_rows),
                                                  C.byref(lv), C.byref(blocks), C.byref(levels), C.byref(widest), C.byref(dropped),
                                                  C.byref(used)))
    level_of_row = np.ctypeslib.as_array(lv, shape=(max(n, 1),))[:n].copy()
    lib().spmv_mi355x_free(lv)
    return dict(level_of_row=level_of_row, blocks=blocks.value, max_block_levels=levels.value, max_level_rows=widest.value,
                nnz_dropped=dropped.value, block_rows=used.value)


def trsv_update_map(row_ptr, col_idx, n, uplo, diag="stored", chain_rows=0, block_rows=None):
    """Where TriangularSolve.update_values takes every stored value from, derived on the host from the pattern alone
    (spmv_mi355x_trsv_update_map): dict(slot_src, slots, diag_src). slot_src[e] is the entry of the given CSR in slot e of the stored
    value array (-1: padding); diag_src[p] the first stored diagonal of the row at position p (None under diag="unit"). block_rows =
    None gives the global form, 0 or a size the blocked one."""
    row_ptr = np.ascontiguousarray(row_ptr, np.int32)
    col_idx = np.ascontiguousarray(col_idx, np.int32)
    ss, ds, slots = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.c_long()
    _check(lib().spmv_mi355x_trsv_update_map(_UPLO[uplo], _DIAG[diag], n, _p(row_ptr), _p(col_idx), chain_rows,
                                             -1 if block_rows is None else block_rows, C.byref(ss), C.byref(slots), C.byref(ds)))
    slot_src = np.ctypeslib.as_array(ss, shape=(max(slots.value, 1),))[:slots.value].copy()
    lib().spmv_mi355x_free(ss)
    diag_src = None
    if ds:
        diag_src = np.ctypeslib.as_array(ds, shape=(max(n, 1),))[:n].copy()
        lib().spmv_mi355x_free(ds)
    return dict(slot_src=slot_src, slots=slots.value, diag_src=diag_src)


class TriangularSolve:
    """T x = b for one triangle of a square CSR matrix (include/spmv_mi355x.h "sparse triangular solve"): uplo "lower" keeps the
    entries with column <= row, "upper" those with column >= row; diag "stored" divides by the stored diagonal, "unit" takes 1 and
    ignores what is stored there. Bit-identical to the sequential loop whatever the plan. block_rows = None gives the global handle;
    0 (the default size) or a size > 0 gives the blocked form, which drops the entries that couple different blocks of block_rows
    rows and solves what is left in one launch (spmv_mi355x_trsv_create_blocked)."""

    def __init__(self, row_ptr, col_idx, values, n, uplo="lower", diag="stored", dtype=np.float64, chain_rows=0, device=-1,
                 block_rows=None, sweeps=0):
        if block_rows is not None and chain_rows != 0:
            raise ValueError("chain_rows belongs to the global plan: it cannot be combined with block_rows")
        row_ptr = np.ascontiguousarray(row_ptr, np.int32)
        col_idx = np.ascontiguousarray(col_idx, np.int32)
        values = np.ascontiguousarray(values, np.float64)
        self.dtype = np.dtype(dtype)
        self.n = int(n)
        self.diag = _DIAG[diag]
        self.h = C.c_void_p()
        if block_rows is None:
            _check(lib().spmv_mi355x_trsv_create(C.byref(self.h), C.c_int(_UPLO[uplo]), C.c_int(_DIAG[diag]),
                                                 F64 if self.dtype == np.float64 else F32, C.c_long(n), _p(row_ptr), _p(col_idx),
                                                 _p(values), C.c_int(chain_rows), C.c_int(device)))
        else:
            _check(lib().spmv_mi355x_trsv_create_blocked(C.byref(self.h), C.c_int(_UPLO[uplo]), C.c_int(_DIAG[diag]),
                                                         F64 if self.dtype == np.float64 else F32, C.c_long(n), _p(row_ptr),
                                                         _p(col_idx), _p(values), C.c_long(block_rows), C.c_int(device)))
        self.mem_footprint = lib().spmv_mi355x_trsv_mem_footprint(self.h)
        if sweeps:
            self.set_sweeps(sweeps)

    def set_sweeps(self, sweeps):
        """sweeps > 0: solve, solve_device, solve_multi*, time_device and time_multi_device of this handle, and with them every
        solver that is given it in a precond triple, run that many Jacobi sweeps in the place of the exact plan; 0 restores the
        exact plan (spmv_mi355x_trsv_set_sweeps). The two handles of an SGS / IC(0) triple need the SAME count under CG."""
        _check(lib().spmv_mi355x_trsv_set_sweeps(self.h, int(sweeps)))

    @property
    def sweeps(self):
        """the setting of set_sweeps (0 = exact)"""
        return self.sweeps_info()["sweeps"]

    def sweeps_info(self, k=1):
        """dict(sweeps, effective, launches, bytes) of spmv_mi355x_trsv_sweeps_info for k columns: the setting, min(setting, levels),
        the launches of one solve under the setting and the map and scratch bytes allocated so far (host only)"""
        setting, effective, launches, nbytes = C.c_int(), C.c_long(), C.c_long(), C.c_double()
        _check(lib().spmv_mi355x_trsv_sweeps_info(self.h, int(k), C.byref(setting), C.byref(effective), C.byref(launches),
                                                  C.byref(nbytes)))
        return dict(sweeps=setting.value, effective=effective.value, launches=launches.value, bytes=nbytes.value)

    def solve_sweeps(self, b, sweeps):
        """x(sweeps) of the Jacobi sweeps x(1) = D^-1 b, x(m + 1) = D^-1 (b - N x(m)) for a host vector b, whatever set_sweeps says;
        from `levels` sweeps on the bits of solve(b) (spmv_mi355x_trsv_solve_sweeps; blocking)"""
        b = np.ascontiguousarray(b, self.dtype)
        if b.shape != (self.n,):
            raise ValueError(f"b must have {self.n} values, got {b.shape}")
        x = np.full(max(self.n, 1), np.nan, self.dtype)
        _check(lib().spmv_mi355x_trsv_solve_sweeps(self.h, int(sweeps), _p(b), _p(x)))
        return x[:self.n]

    def solve_sweeps_device(self, b_ptr, x_ptr, sweeps, stream=None):
        """The same on device pointers (b_ptr == x_ptr: in place), enqueued on `stream`; x holds intermediate sweeps until the solve
        has finished (spmv_mi355x_trsv_solve_sweeps_device_async)"""
        _check(lib().spmv_mi355x_trsv_solve_sweeps_device_async(self.h, int(sweeps), C.c_void_p(b_ptr), C.c_void_p(x_ptr),
                                                                C.c_void_p(stream or 0)))

    def solve_sweeps_multi(self, B, sweeps):
        """The sweeps on a host block B of shape (n, k), column j bit-identical to solve_sweeps(B[:, j], sweeps)
        (spmv_mi355x_trsv_solve_sweeps_multi; blocking)"""
        B = np.ascontiguousarray(B, self.dtype)
        if B.ndim != 2 or B.shape[0] != self.n or B.shape[1] < 1:
            raise ValueError(f"B must have shape ({self.n}, k) with k >= 1, got {B.shape}")
        k = B.shape[1]
        X = np.full((max(self.n, 1), k), np.nan, self.dtype)
        _check(lib().spmv_mi355x_trsv_solve_sweeps_multi(self.h, int(sweeps), k, _p(B), _p(X)))
        return X[:self.n]

    def solve_sweeps_multi_device(self, k, b_ptr, ldb, x_ptr, ldx, sweeps, stream=None):
        """The same on device pointers of row-major blocks (row i at ptr + i * ld values; b_ptr == x_ptr with ldb == ldx: in place),
        enqueued on `stream` (spmv_mi355x_trsv_solve_sweeps_multi_device_async)"""
        _check(lib().spmv_mi355x_trsv_solve_sweeps_multi_device_async(self.h, int(sweeps), k, C.c_void_p(b_ptr), ldb, C.c_void_p(x_ptr),
                                                                      ldx, C.c_void_p(stream or 0)))

    @property
    def info(self):
        """dict(n, nnz_kept, levels, launches, max_level_rows, chain_rows) of spmv_mi355x_trsv_info"""
        n, kept, levels, launches, widest, chain = C.c_long(), C.c_long(), C.c_long(), C.c_long(), C.c_long(), C.c_int()
        _check(lib().spmv_mi355x_trsv_info(self.h, C.byref(n), C.byref(kept), C.byref(levels), C.byref(launches), C.byref(widest),
                                           C.byref(chain)))
        return dict(n=n.value, nnz_kept=kept.value, levels=levels.value, launches=launches.value, max_level_rows=widest.value,
                    chain_rows=chain.value)

    def block_info(self):
        """dict(block_rows, blocks, max_block_levels, nnz_dropped) of spmv_mi355x_trsv_block_info; all 0 for a global handle"""
        rows, blocks, levels, dropped = C.c_long(), C.c_long(), C.c_long(), C.c_long()
        _check(lib().spmv_mi355x_trsv_block_info(self.h, C.byref(rows), C.byref(blocks), C.byref(levels), C.byref(dropped)))
        return dict(block_rows=rows.value, blocks=blocks.value, max_block_levels=levels.value, nnz_dropped=dropped.value)

    def solve(self, b):
        """x of T x = b for a host vector b of n values (spmv_mi355x_trsv_solve; blocking)"""
        b = np.ascontiguousarray(b, self.dtype)
        if b.shape != (self.n,):
            raise ValueError(f"b must have {self.n} values, got {b.shape}")
        x = np.full(max(self.n, 1), np.nan, self.dtype)
        _check(lib().spmv_mi355x_trsv_solve(self.h, _p(b), _p(x)))
        return x[:self.n]

    def solve_device(self, b_ptr, x_ptr, stream=None):
        """The same on device pointers (b_ptr == x_ptr: in place), enqueued on `stream` (spmv_mi355x_trsv_solve_device_async)"""
        _check(lib().spmv_mi355x_trsv_solve_device_async(self.h, C.c_void_p(b_ptr), C.c_void_p(x_ptr), C.c_void_p(stream or 0)))

    def time_device(self, b_ptr, x_ptr, iters, stream=None):
        """ms per solve of `iters` back-to-back solves, timed with HIP events on `stream` (spmv_mi355x_time_trsv_device)"""
        ms = C.c_double()
        _check(lib().spmv_mi355x_time_trsv_device(self.h, C.c_void_p(b_ptr), C.c_void_p(x_ptr), C.c_int(iters), C.c_void_p(stream or 0),
                                                  C.byref(ms)))
        return ms.value

    def solve_multi(self, B):
        """X of T X = B for a host block B of shape (n, k), column j bit-identical to solve(B[:, j]) (spmv_mi355x_trsv_solve_multi;
        blocking)"""
        B = np.ascontiguousarray(B, self.dtype)
        if B.ndim != 2 or B.shape[0] != self.n or B.shape[1] < 1:
            raise ValueError(f"B must have shape ({self.n}, k) with k >= 1, got {B.shape}")
        k = B.shape[1]
        X = np.full((max(self.n, 1), k), np.nan, self.dtype)
        _check(lib().spmv_mi355x_trsv_solve_multi(self.h, k, _p(B), _p(X)))
        return X[:self.n]

    def solve_multi_device(self, k, b_ptr, ldb, x_ptr, ldx, stream=None):
        """The same on device pointers of row-major blocks (row i at ptr + i * ld values; b_ptr == x_ptr with ldb == ldx: in place),
        enqueued on `stream` (spmv_mi355x_trsv_solve_multi_device_async)"""
        _check(lib().spmv_mi355x_trsv_solve_multi_device_async(self.h, k, C.c_void_p(b_ptr), ldb, C.c_void_p(x_ptr), ldx,
                                                               C.c_void_p(stream or 0)))

    def solve_multi_plan(self, k):
        """dict(matrix_passes, launches, max_chunk) of a k-column solve (spmv_mi355x_trsv_solve_multi_plan; host only)"""
        passes, launches, widest = C.c_long(), C.c_long(), C.c_int()
        _check(lib().spmv_mi355x_trsv_solve_multi_plan(self.h, k, C.byref(passes), C.byref(launches), C.byref(widest)))
        return dict(matrix_passes=passes.value, launches=launches.value, max_chunk=widest.value)

    def time_multi_device(self, k, b_ptr, ldb, x_ptr, ldx, iters, stream=None):
        """ms per k-column solve of `iters` back-to-back solves, timed with HIP events (spmv_mi355x_time_trsv_multi_device)"""
        ms = C.c_double()
        _check(lib().spmv_mi355x_time_trsv_multi_device(self.h, k, C.c_void_p(b_ptr), ldb, C.c_void_p(x_ptr), ldx, iters,
                                                        C.c_void_p(stream or 0), C.byref(ms)))
        return ms.value

    def update_values_prepare(self, row_ptr, col_idx):
        """Once per handle: derive and upload the entry map from the CSR the handle was created with, which also fixes the entry
        order of every later values array (spmv_mi355x_trsv_update_values_prepare). A second call does nothing."""
        row_ptr = np.ascontiguousarray(row_ptr, np.int32)
        col_idx = np.ascontiguousarray(col_idx, np.int32)
        _check(lib().spmv_mi355x_trsv_update_values_prepare(self.h, self.n, _p(row_ptr), _p(col_idx)))
        self._update_nnz = int(row_ptr[self.n])
        return self

    def update_values(self, values):
        """New host values in the entry order of prepare's CSR; the handle becomes byte for byte what the constructor builds from
        them (spmv_mi355x_trsv_update_values; blocking). A zero or non-finite new diagonal raises, names the row and leaves the
        previous values in place."""
        values = np.ascontiguousarray(values, np.float64)
        nnz = getattr(self, "_update_nnz", None)
        if nnz is not None and values.shape != (nnz,):
            raise ValueError(f"values must have {nnz} entries, got {values.shape}")
        _check(lib().spmv_mi355x_trsv_update_values(self.h, _p(values)))
        return self

    def update_values_device(self, ptr, stream=None, wait=True):
        """The same from a device pointer to fp64 values, enqueued on `stream`. wait=True (spmv_mi355x_trsv_update_values_device)
        blocks and raises on a refusal; wait=False (spmv_mi355x_trsv_update_values_device_async) returns at once: the refusal is then
        decided on the device alone and update_values_result() reports it. Solves of this handle must be ordered behind the update
        through the stream."""
        fn = lib().spmv_mi355x_trsv_update_values_device if wait else lib().spmv_mi355x_trsv_update_values_device_async
        _check(fn(self.h, C.c_void_p(ptr), C.c_void_p(stream or 0)))
        return self

    def update_values_result(self):
        """Waits for the last async update: -1 when it was accepted, else the lowest refused row, the handle holding the values from
        before it (spmv_mi355x_trsv_update_values_result; the message is in spmv_mi355x_last_error)"""
        bad = C.c_long(-1)
        rc = lib().spmv_mi355x_trsv_update_values_result(self.h, C.byref(bad))
        if rc != 0 and bad.value < 0:
            _check(rc)
        return bad.value

    @property
    def update_values_state(self):
        """1 = update_values_prepare is missing, 2 = ready, 3 = the last update was refused (spmv_mi355x_trsv_update_values_state)"""
        return lib().spmv_mi355x_trsv_update_values_state(self.h)

    @property
    def update_values_bytes(self):
        """device bytes of the entry maps and the status block, which mem_footprint does not count; 0 before prepare"""
        return lib().spmv_mi355x_trsv_update_values_bytes(self.h)

    def stored_values(self):
        """(val, diag): the stored value array, padding included, and the diagonal by position, both in the handle's precision; diag
        is None under diag="unit" (spmv_mi355x_trsv_stored_values; blocking)"""
        slots = C.c_long()
        _check(lib().spmv_mi355x_trsv_stored_values(self.h, None, C.byref(slots), None))
        val = np.zeros(max(slots.value, 1), self.dtype)
        diag = np.zeros(max(self.n, 1), self.dtype) if self.diag == DIAG_STORED else None
        _check(lib().spmv_mi355x_trsv_stored_values(self.h, _p(val), C.byref(slots), None if diag is None else _p(diag)))
        return val[:slots.value], None if diag is None else diag[:self.n]

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            lib().spmv_mi355x_trsv_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sgs_precond(row_ptr, col_idx, values, n, dtype=np.float64, block_rows=None, **trsv_opts):
    """(first, scale, second) of the symmetric Gauss-Seidel preconditioner of A for Matrix.gmres(precond=...) and Matrix.pcg_tri:
    the LOWER / STORED and UPPER / STORED TriangularSolve handles of A's CSR with diag(A) as the scale between them. block_rows =
    None gives global handles, otherwise blocked handles with that size on both sides (the same size keeps M symmetric). The
    diagonal is the first stored entry of row i with column i, the solvers' rule. trsv_opts go to both TriangularSolve handles
    (chain_rows, device). The caller closes the two handles."""
    row_ptr = np.ascontiguousarray(row_ptr, np.int32)
    col_idx = np.ascontiguousarray(col_idx, np.int32)
    values = np.ascontiguousarray(values, np.float64)
    rows = np.repeat(np.arange(n), np.diff(row_ptr))
    at = np.nonzero(col_idx == rows)[0]
    at = at[np.unique(rows[at], return_index=True)[1]]               # the first of every row
    if at.size != n:
        raise ValueError(f"sgs_precond: {n - at.size} rows store no diagonal entry")
    first = TriangularSolve(row_ptr, col_idx, values, n, uplo="lower", dtype=dtype, block_rows=block_rows, **trsv_opts)
    second = TriangularSolve(row_ptr, col_idx, values, n, uplo="upper", dtype=dtype, block_rows=block_rows, **trsv_opts)
    return first, values[at].astype(dtype), second


def sgs_precond_update(precond, row_ptr, col_idx, values):
    """New values of A, same pattern, for the triple sgs_precond returned: both handles are prepared on first use and updated from
    ONE upload of `values` (TriangularSolve.update_values_device), the scale array is rewritten in place with the new first-stored
    diagonals. Returns the triple. A zero or non-finite new diagonal raises before anything is written: both handles check the same
    diagonals and each keeps its previous values."""
    first, scale, second = precond
    row_ptr = np.ascontiguousarray(row_ptr, np.int32)
    col_idx = np.ascontiguousarray(col_idx, np.int32)
    values = np.ascontiguousarray(values, np.float64)
    n = first.n
    rows = np.repeat(np.arange(n), np.diff(row_ptr))
    at = np.nonzero(col_idx == rows)[0]
    at = at[np.unique(rows[at], return_index=True)[1]]               # the first of every row
    first.update_values_prepare(row_ptr, col_idx)
    second.update_values_prepare(row_ptr, col_idx)
    first.update_values(values)                                      # the one upload: the handle's staging buffer
    staged = C.c_void_p()
    _check(lib().spmv_mi355x_trsv_update_values_staged(first.h, C.byref(staged)))
    second.update_values_device(staged.value or 0, wait=True)
    scale[:] = values[at].astype(scale.dtype)
    return first, scale, second


class Ilu0Info(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("n", C.c_long), ("nnz", C.c_long), ("nnz_dropped", C.c_long), ("levels", C.c_long),
                ("launches", C.c_long), ("max_level_rows", C.c_long), ("block_rows", C.c_long), ("blocks", C.c_long),
                ("breakdown_row", C.c_long), ("factorizations", C.c_long)]


class Ilu0:
    """The ILU(0) factorization of a square matrix on its own pattern, computed on the GPU in fp64 (include/spmv_mi355x.h "ILU(0)"):
    built from the pattern (columns strictly ascending, a stored diagonal in every row), factor(values) any number of times. values()
    is ONE array in A's entry order, unit L strictly below the diagonal and U on and above it, bit-identical to the sequential loop.
    block_rows = None gives the global factorization; 0 (the default size) or a size > 0 the blocked form, which ignores the entries
    that couple different blocks of block_rows rows. precond() gives the triple Matrix.pcg_tri, pcg_trsm_multi and gmres take."""

    def __init__(self, row_ptr, col_idx, n, block_rows=None, device=-1):
        self.row_ptr = np.ascontiguousarray(row_ptr, np.int32)
        self.col_idx = np.ascontiguousarray(col_idx, np.int32)
        self.n = int(n)
        self.block_rows = block_rows
        self.device = device
        self.h = C.c_void_p()
        _check(lib().spmv_mi355x_ilu0_create(C.byref(self.h), C.c_long(n), _p(self.row_ptr), _p(self.col_idx),
                                             C.c_long(-1 if block_rows is None else block_rows), C.c_int(device)))
        self.nnz = int(self.row_ptr[n]) if len(self.row_ptr) else 0
        self.mem_footprint = lib().spmv_mi355x_ilu0_mem_footprint(self.h)

    def factor(self, values):
        """factorize the host values, nnz doubles in A's entry order (spmv_mi355x_ilu0_factor; blocking)"""
        values = np.ascontiguousarray(values, np.float64)
        if values.shape != (self.nnz,):
            raise ValueError(f"values must have {self.nnz} entries, got {values.shape}")
        _check(lib().spmv_mi355x_ilu0_factor(self.h, _p(values)))
        return self

    def factor_device(self, ptr, stream=None):
        """The same on a device pointer, enqueued on `stream` (spmv_mi355x_ilu0_factor_device_async)"""
        _check(lib().spmv_mi355x_ilu0_factor_device_async(self.h, C.c_void_p(ptr), C.c_void_p(stream or 0)))
        return self

    def values(self):
        """f on the host: nnz doubles in A's entry order (spmv_mi355x_ilu0_values; blocking)"""
        out = np.full(max(self.nnz, 1), np.nan)
        _check(lib().spmv_mi355x_ilu0_values(self.h, _p(out)))
        return out[:self.nnz]

    def values_device(self):
        """the device pointer of f (spmv_mi355x_ilu0_values_device): valid until close(), overwritten by the next factor"""
        ptr = C.c_void_p()
        _check(lib().spmv_mi355x_ilu0_values_device(self.h, C.byref(ptr)))
        return ptr.value or 0

    @property
    def info(self):
        """dict(n, nnz, nnz_dropped, levels, launches, max_level_rows, block_rows, blocks, breakdown_row, factorizations) of
        spmv_mi355x_ilu0_get_info; reads the breakdown word, so it synchronises"""
        r = Ilu0Info()
        r.struct_size = C.sizeof(Ilu0Info)
        _check(lib().spmv_mi355x_ilu0_get_info(self.h, C.byref(r)))
        return {k: getattr(r, k) for k, _ in Ilu0Info._fields_ if k != "struct_size"}

    def precond(self, dtype=np.float64, **trsv_opts):
        """(first, None, second) for Matrix.pcg_tri, pcg_trsm_multi and gmres(precond=...): the LOWER / UNIT and UPPER / STORED
        TriangularSolve handles over the factor's CSR, blocked with the factorization's block size when it is blocked. A breakdown
        surfaces here as trsv_create's refusal of the bad diagonal, which names the row. The caller closes the two handles."""
        f = self.values()
        B = None if self.block_rows is None else self.info["block_rows"]
        trsv_opts.setdefault("device", self.device)
        first = TriangularSolve(self.row_ptr, self.col_idx, f, self.n, uplo="lower", diag="unit", dtype=dtype, block_rows=B,
                                **trsv_opts)
        try:
            second = TriangularSolve(self.row_ptr, self.col_idx, f, self.n, uplo="upper", diag="stored", dtype=dtype, block_rows=B,
                                     **trsv_opts)
        except Exception:
            first.close()
            raise
        return first, None, second

    def update_precond(self, precond, stream=None, wait=True):
        """Refresh the triple precond() returned with the factor this handle holds NOW (after a later factor / factor_device): both
        TriangularSolve handles are prepared on first use with the factor's own pattern and updated from values_device(), enqueued
        on `stream`; no host copy of f is made and nothing is analysed or laid out again. Returns the triple.
        A breakdown surfaces as the UPPER handle's refusal, which names the row: `second` is therefore updated first, and when it
        refused, `first` (LOWER / UNIT, which cannot refuse) is skipped, so both handles keep solving with the previous factor.
        wait=False enqueues both updates and returns at once: the guard is then the device-side one alone (`second` keeps its values
        when a pivot is bad, `first` is updated regardless) and the caller must ask second.update_values_result() before trusting
        the pair. Solves must be ordered behind the updates through the stream."""
        first, _, second = precond
        for T in (first, second):
            T.update_values_prepare(self.row_ptr, self.col_idx)
        f = self.values_device()
        second.update_values_device(f, stream, wait)
        first.update_values_device(f, stream, wait)
        return precond

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            lib().spmv_mi355x_ilu0_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ilu0_precond(row_ptr, col_idx, values, n, dtype=np.float64, block_rows=None, **trsv_opts):
    """(first, None, second) of the ILU(0) preconditioner of A, factorized on the GPU: the one-call form of Ilu0(...).factor(values)
    .precond(dtype), beside sgs_precond. For a symmetric positive definite A this is IC(0)'s M. `device` of trsv_opts also places the
    factorization. The caller closes the two handles."""
    F = Ilu0(row_ptr, col_idx, n, block_rows=block_rows, device=trsv_opts.pop("device", -1))
    try:
        return F.factor(values).precond(dtype, **trsv_opts)
    finally:
        F.close()


COLOR_FORWARD, COLOR_BACKWARD = 0, 1


class ColorStats(C.Structure):
    _fields_ = [("struct_size", C.c_size_t), ("n", C.c_long), ("nnz", C.c_long), ("symmetric", C.c_long), ("num_colors", C.c_long),
                ("rounds", C.c_long), ("max_class", C.c_long), ("min_class", C.c_long), ("transpose_seconds", C.c_double),
                ("round_seconds", C.c_double), ("sort_seconds", C.c_double), ("permute_seconds", C.c_double)]


class Coloring:
    """A multicolouring of the graph of a square CSR pattern (a_ij or a_ji stored), computed on the GPU, and the permutation that sorts
    the rows by colour (include/spmv_mi355x.h "multicolour ordering"). colors[i] is the colour of row i, equal to first-fit greedy
    colouring in descending key order; perm[p] is the old row at new position p, rank its inverse, color_ptr the first position of
    every colour. permute_csr gives B = P A P^t, whose triangles have as many levels as there are colours: TriangularSolve, Ilu0,
    sgs_precond, ilu0_precond and Matrix are then used on B as on any matrix, with permute(b) going in and unpermute(x) coming out."""

    def __init__(self, row_ptr, col_idx, n, device=-1):
        row_ptr = np.ascontiguousarray(row_ptr, np.int32)
        col_idx = np.ascontiguousarray(col_idx, np.int32)
        self.n = int(n)
        self.h = C.c_void_p()
        _check(lib().spmv_mi355x_color_create(C.byref(self.h), C.c_long(n), _p(row_ptr), _p(col_idx), C.c_int(device)))
        self.nnz = int(row_ptr[n]) if len(row_ptr) else 0
        st = self.info()
        self.num_colors = st["num_colors"]
        self.colors = np.full(max(self.n, 1), -1, np.int32)
        self.perm = np.full(max(self.n, 1), -1, np.int32)
        self.rank = np.full(max(self.n, 1), -1, np.int32)
        self.color_ptr = np.full(self.num_colors + 1, -1, np.int32)
        _check(lib().spmv_mi355x_color_colors(self.h, _p(self.colors)))
        _check(lib().spmv_mi355x_color_perm(self.h, _p(self.perm), _p(self.rank)))
        _check(lib().spmv_mi355x_color_color_ptr(self.h, _p(self.color_ptr)))
        self.colors, self.perm, self.rank = self.colors[:self.n], self.perm[:self.n], self.rank[:self.n]

    @property
    def mem_footprint(self):
        return lib().spmv_mi355x_color_mem_footprint(self.h)

    def info(self):
        """dict(n, nnz, symmetric, num_colors, rounds, max_class, min_class, transpose_seconds, round_seconds, sort_seconds,
        permute_seconds) of spmv_mi355x_color_info"""
        r = ColorStats()
        r.struct_size = C.sizeof(ColorStats)
        _check(lib().spmv_mi355x_color_info(self.h, C.byref(r)))
        return {k: getattr(r, k) for k, _ in ColorStats._fields_ if k != "struct_size"}

    def permute_csr(self, values=None):
        """(row_ptr, col_idx, values, entry_map) of B = P A P^t on the host: row p holds row perm[p] of A with columns rank[j] in
        ascending new column order, equal columns in stored order; values_B = values_A[entry_map] (None without values)
        (spmv_mi355x_color_permute_csr; blocking)"""
        rp = np.zeros(self.n + 1, np.int32)
        ci = np.zeros(max(self.nnz, 1), np.int32)
        em = np.zeros(max(self.nnz, 1), np.int32)
        va = out = None
        if values is not None:
            va = np.ascontiguousarray(values, np.float64)
            if va.shape != (self.nnz,):
                raise ValueError(f"values must have {self.nnz} entries, got {va.shape}")
            out = np.full(max(self.nnz, 1), np.nan)
        _check(lib().spmv_mi355x_color_permute_csr(self.h, None if va is None else _p(va), _p(rp), _p(ci), None if out is None else _p(out),
                                                   _p(em)))
        return rp, ci[:self.nnz], None if out is None else out[:self.nnz], em[:self.nnz]

    def permute_csr_device(self):
        """(row_ptr, col_idx, entry_map) of B as device pointers the handle owns, valid until close()
        (spmv_mi355x_color_permute_csr_device)"""
        rp, ci, em = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().spmv_mi355x_color_permute_csr_device(self.h, C.byref(rp), C.byref(ci), C.byref(em)))
        return rp.value or 0, ci.value or 0, em.value or 0

    def permute_values(self, values):
        """values_A[entry_map] for host values (spmv_mi355x_color_permute_values; blocking)"""
        values = np.ascontiguousarray(values, np.float64)
        if values.shape != (self.nnz,):
            raise ValueError(f"values must have {self.nnz} entries, got {values.shape}")
        out = np.full(max(self.nnz, 1), np.nan)
        _check(lib().spmv_mi355x_color_permute_values(self.h, _p(values), _p(out)))
        return out[:self.nnz]

    def permute_values_device(self, in_ptr, out_ptr, stream=None):
        """The same gather on device pointers to nnz doubles each, enqueued on `stream`
        (spmv_mi355x_color_permute_values_device_async): out is what update_values_device of a handle of B, Ilu0.factor_device and
        TriangularSolve.update_values_device take"""
        _check(lib().spmv_mi355x_color_permute_values_device_async(self.h, C.c_void_p(in_ptr), C.c_void_p(out_ptr), C.c_void_p(stream or 0)))

    def _vectors(self, direction, V):
        V = np.asarray(V)
        if V.dtype not in (np.float32, np.float64):
            V = V.astype(np.float64)
        V = np.ascontiguousarray(V)
        if V.ndim not in (1, 2) or V.shape[0] != self.n:
            raise ValueError(f"expected {self.n} rows, got {V.shape}")
        k = 1 if V.ndim == 1 else V.shape[1]
        out = np.full_like(V, np.nan) if V.size else V.copy()
        if V.size:
            _check(lib().spmv_mi355x_color_permute_vectors(self.h, C.c_int(direction), C.c_int(F32 if V.dtype == np.float32 else F64),
                                                           C.c_int(k), _p(V), C.c_long(k), _p(out), C.c_long(k)))
        return out

    def permute(self, V):
        """V[perm] for a host vector of n values or an n x k block, fp32 or fp64: into the colour ordering
        (spmv_mi355x_color_permute_vectors, forward; blocking)"""
        return self._vectors(COLOR_FORWARD, V)

    def unpermute(self, V):
        """the inverse of permute: out[perm[p]] = V[p], back into the caller's ordering"""
        return self._vectors(COLOR_BACKWARD, V)

    def permute_device(self, in_ptr, out_ptr, k=1, dtype=np.float64, ldin=None, ldout=None, stream=None, direction=COLOR_FORWARD):
        """The same on device pointers to row-major n x k blocks with leading dimensions ldin / ldout (default k), enqueued on
        `stream` (spmv_mi355x_color_permute_vectors_device_async); in_ptr == out_ptr is refused"""
        _check(lib().spmv_mi355x_color_permute_vectors_device_async(
            self.h, C.c_int(direction), C.c_int(F32 if np.dtype(dtype) == np.float32 else F64), C.c_int(k), C.c_void_p(in_ptr),
            C.c_long(k if ldin is None else ldin), C.c_void_p(out_ptr), C.c_long(k if ldout is None else ldout), C.c_void_p(stream or 0)))

    def unpermute_device(self, in_ptr, out_ptr, k=1, dtype=np.float64, ldin=None, ldout=None, stream=None):
        self.permute_device(in_ptr, out_ptr, k, dtype, ldin, ldout, stream, COLOR_BACKWARD)

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            lib().spmv_mi355x_color_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def multicolor_system(row_ptr, col_idx, values, n, device=-1):
    """(coloring, row_ptr_B, col_idx_B, values_B) of B = P A P^t under the multicolouring of A's graph: sgs_precond, ilu0_precond, Ilu0,
    TriangularSolve and Matrix are called on B exactly as on A; A x = b becomes B (P x) = P b, i.e. x = coloring.unpermute(the
    solution for coloring.permute(b)). The caller closes the coloring."""
    col = Coloring(row_ptr, col_idx, n, device=device)
    try:
        rp, ci, va, _ = col.permute_csr(values)
    except Exception:
        col.close()
        raise
    return col, rp, ci, va


FSAI_MAX_ROW = 128


def fsai_pattern(row_ptr, col_idx, n, power=1):
    """(row_ptr, col_idx) of the pattern of tril(A~)^power, A~ = the lower triangle of A's pattern with the diagonal added, columns
    ascending (spmv_mi355x_fsai_pattern; host only). power is 1, 2 or 3."""
    row_ptr = np.ascontiguousarray(row_ptr, np.int32)
    col_idx = np.ascontiguousarray(col_idx, np.int32)
    rp, ci = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)()
    _check(lib().spmv_mi355x_fsai_pattern(C.c_long(n), _p(row_ptr), _p(col_idx), C.c_int(power), C.byref(rp), C.byref(ci)))
    out_rp = np.ctypeslib.as_array(rp, shape=(n + 1,)).copy()
    out_ci = np.ctypeslib.as_array(ci, shape=(max(int(out_rp[n]), 1),))[:out_rp[n]].copy()
    lib().spmv_mi355x_free(rp)
    lib().spmv_mi355x_free(ci)
    return out_rp, out_ci


class Fsai:
    """The factorized sparse approximate inverse of a symmetric positive definite matrix (include/spmv_mi355x.h "FSAI"): a lower
    triangular G on `pattern` = (row_ptr, col_idx), or on the lower triangle of A's own pattern when None, with G A G^t ~ I, built
    on the GPU. apply(v) is G^t (G v), two SpMVs over the handles G and Gt, which are built in `fmt` with `opts`.
    Matrix.pcg_tri(b, precond=<Fsai>) preconditions CG with it."""

    def __init__(self, row_ptr, col_idx, values, n, pattern=None, fmt="sell_c_sigma", dtype=np.float64, **opts):
        row_ptr = np.ascontiguousarray(row_ptr, np.int32)
        col_idx = np.ascontiguousarray(col_idx, np.int32)
        values = np.ascontiguousarray(values, np.float64)
        prp = pci = None
        if pattern is not None:
            prp = np.ascontiguousarray(pattern[0], np.int32)
            pci = np.ascontiguousarray(pattern[1], np.int32)
        self.dtype = np.dtype(dtype)
        self.n = int(n)
        self.h = C.c_void_p()
        o = _make_opts(opts)
        fmt_id = FORMATS[fmt] if isinstance(fmt, str) else fmt
        _check(lib().spmv_mi355x_fsai_create(C.byref(self.h), fmt_id, F64 if self.dtype == np.float64 else F32, C.c_long(n),
                                             _p(row_ptr), _p(col_idx), _p(values), None if prp is None else _p(prp),
                                             None if pci is None else _p(pci), C.byref(o)))
        self.mem_footprint = lib().spmv_mi355x_fsai_mem_footprint(self.h)
        g, gt = C.c_void_p(), C.c_void_p()
        _check(lib().spmv_mi355x_fsai_matrices(self.h, C.byref(g), C.byref(gt)))
        # Matrix objects over the borrowed handles: they never destroy them (close() of a borrowed Matrix only forgets the handle)
        self.G = Matrix(None, None, None, 0, 0, fmt, dtype, _handle=g, _borrowed=True) if g else None
        self.Gt = Matrix(None, None, None, 0, 0, fmt, dtype, _handle=gt, _borrowed=True) if gt else None

    def info(self):
        """dict(n, nnz, max_row, fallback_rows, kernel_seconds, setup_seconds, download_seconds, create_g_seconds,
        create_gt_seconds) of spmv_mi355x_fsai_info and spmv_mi355x_fsai_setup_split"""
        n, nnz, widest, fell = C.c_long(), C.c_long(), C.c_long(), C.c_long()
        kernel, setup, down, cg, cgt = C.c_double(), C.c_double(), C.c_double(), C.c_double(), C.c_double()
        _check(lib().spmv_mi355x_fsai_info(self.h, C.byref(n), C.byref(nnz), C.byref(widest), C.byref(fell), C.byref(kernel),
                                           C.byref(setup)))
        _check(lib().spmv_mi355x_fsai_setup_split(self.h, None, C.byref(down), C.byref(cg), C.byref(cgt)))
        return dict(n=n.value, nnz=nnz.value, max_row=widest.value, fallback_rows=fell.value, kernel_seconds=kernel.value,
                    setup_seconds=setup.value, download_seconds=down.value, create_g_seconds=cg.value, create_gt_seconds=cgt.value)

    def values(self):
        """G's values in fp64, in the pattern's entry order, whatever the handle's precision"""
        out = np.zeros(max(self.info()["nnz"], 1))
        _check(lib().spmv_mi355x_fsai_values(self.h, _p(out)))
        return out[:self.info()["nnz"]]

    def apply(self, v):
        """G^t (G v) for a host vector of n values (spmv_mi355x_fsai_apply; blocking)"""
        v = np.ascontiguousarray(v, self.dtype)
        if v.shape != (self.n,):
            raise ValueError(f"v must have {self.n} values, got {v.shape}")
        out = np.full(max(self.n, 1), np.nan, self.dtype)
        _check(lib().spmv_mi355x_fsai_apply(self.h, _p(v), _p(out)))
        return out[:self.n]

    def apply_device(self, in_ptr, out_ptr, stream=None):
        """The same on device pointers (in_ptr == out_ptr: in place), enqueued on `stream` (spmv_mi355x_fsai_apply_device_async)"""
        _check(lib().spmv_mi355x_fsai_apply_device_async(self.h, C.c_void_p(in_ptr), C.c_void_p(out_ptr), C.c_void_p(stream or 0)))

    def apply_multi(self, V):
        """G^t (G V) for the k columns of a host block of shape (n, k) (spmv_mi355x_fsai_apply_multi; blocking): column j holds the
        bits of apply(V[:, j]) on a deterministic layout"""
        V = np.ascontiguousarray(V, self.dtype)
        if V.ndim != 2 or V.shape[0] != self.n or V.shape[1] < 1:
            raise ValueError(f"V must have shape ({self.n}, k) with k >= 1, got {V.shape}")
        out = np.zeros(V.shape, self.dtype)
        _check(lib().spmv_mi355x_fsai_apply_multi(self.h, V.shape[1], _p(V), _p(out)))
        return out

    def apply_multi_device(self, k, in_ptr, ldin, out_ptr, ldout, stream=None):
        """The same on device blocks, row i at ptr + i * ld values (in_ptr == out_ptr with ldin == ldout: in place), enqueued on
        `stream` (spmv_mi355x_fsai_apply_multi_device_async)"""
        _check(lib().spmv_mi355x_fsai_apply_multi_device_async(self.h, k, in_ptr, ldin, out_ptr, ldout, stream or 0))

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            for M in (self.G, self.Gt):
                if M is not None:
                    M.close()
            lib().spmv_mi355x_fsai_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class AmgOpts(C.Structure):
    """spmv_mi355x_amg_opts (include/spmv_mi355x.h "AMG")"""
    _fields_ = [("struct_size", C.c_int), ("theta", C.c_double), ("max_levels", C.c_int), ("coarse_rows", C.c_int),
                ("sweeps", C.c_int), ("coarse_sweeps", C.c_int)]


AMG_MAX_LEVELS = 16
AMG_DEFAULTS = dict(theta=0.08, max_levels=10, coarse_rows=128, sweeps=1, coarse_sweeps=4)
AMG_COARSE_KINDS = ("dense", "sweeps", "sweeps after a failed pivot")
AMG_A, AMG_P, AMG_AF = 0, 1, 2


class AmgStats(C.Structure):
    """spmv_mi355x_amg_stats (include/spmv_mi355x.h "AMG")"""
    _fields_ = [("struct_size", C.c_uint), ("levels", C.c_int), ("coarse_kind", C.c_int), ("stalled", C.c_int),
                ("rows", C.c_long * AMG_MAX_LEVELS), ("nnz", C.c_long * AMG_MAX_LEVELS), ("nnz_p", C.c_long * AMG_MAX_LEVELS),
                ("aggregates", C.c_long * AMG_MAX_LEVELS), ("mis_rounds", C.c_long * AMG_MAX_LEVELS),
                ("omega", C.c_double * AMG_MAX_LEVELS), ("rho", C.c_double * AMG_MAX_LEVELS),
                ("operator_complexity", C.c_double), ("grid_complexity", C.c_double),
                ("spmvs_per_apply", C.c_long), ("launches_per_apply", C.c_long),
                ("setup_seconds", C.c_double), ("coarsen_seconds", C.c_double), ("spgemm_seconds", C.c_double),
                ("transpose_seconds", C.c_double), ("create_seconds", C.c_double), ("download_seconds", C.c_double)]


class AmgProlongatorOpts(C.Structure):
    """spmv_mi355x_amg_prolongator_opts (include/spmv_mi355x.h "AMG: a caller's near-null vector and filtered prolongator smoothing")"""
    _fields_ = [("struct_size", C.c_int), ("filtered", C.c_int), ("near_null", C.c_void_p)]


class AmgProlongatorStats(C.Structure):
    """spmv_mi355x_amg_prolongator_stats"""
    _fields_ = [("struct_size", C.c_uint), ("filtered", C.c_int), ("has_near_null", C.c_int),
                ("nnz_filtered", C.c_long * AMG_MAX_LEVELS), ("unfiltered_rows", C.c_long * AMG_MAX_LEVELS),
                ("omega_p", C.c_double * AMG_MAX_LEVELS), ("rho_p", C.c_double * AMG_MAX_LEVELS)]


class AmgUpdateStats(C.Structure):
    """spmv_mi355x_amg_update_stats (include/spmv_mi355x.h "AMG: new values for a hierarchy")"""
    _fields_ = [("struct_size", C.c_uint), ("prepared", C.c_int), ("failed", C.c_int), ("updates", C.c_long),
                ("prepare_bytes", C.c_double), ("prepare_seconds", C.c_double),
                ("update_seconds", C.c_double), ("spgemm_seconds", C.c_double), ("handle_seconds", C.c_double)]


class AmgFoldStats(C.Structure):
    """spmv_mi355x_amg_fold_stats (include/spmv_mi355x.h "AMG: the small levels as one launch")"""
    _fields_ = [("struct_size", C.c_uint), ("fold_rows", C.c_int), ("first_level", C.c_int), ("folded_levels", C.c_int),
                ("launches_per_apply", C.c_long), ("spmvs_per_apply", C.c_long), ("tail_products", C.c_long), ("tail_entries", C.c_long),
                ("lanes_per_row", C.c_int * AMG_MAX_LEVELS), ("bytes", C.c_double)]


class Amg:
    """The smoothed-aggregation multilevel preconditioner of a symmetric positive definite matrix (include/spmv_mi355x.h "AMG"),
    built on the GPU: apply(v) is one V(sweeps, sweeps) cycle over handles built in `fmt` with `opts`. `.A` is the borrowed handle of
    A itself, `.levels` the number of levels. Matrix.pcg_tri(b, precond=<Amg>) preconditions CG with it. Amg.build(...) is the same
    with a caller's near-null vector and / or filtered prolongator smoothing (spmv_mi355x_amg_create_with)."""

    def __init__(self, row_ptr, col_idx, values, n, fmt="sell_c_sigma", dtype=np.float64, theta=AMG_DEFAULTS["theta"],
                 max_levels=AMG_DEFAULTS["max_levels"], coarse_rows=AMG_DEFAULTS["coarse_rows"], sweeps=AMG_DEFAULTS["sweeps"],
                 coarse_sweeps=AMG_DEFAULTS["coarse_sweeps"], **opts):
        row_ptr = np.ascontiguousarray(row_ptr, np.int32)
        col_idx = np.ascontiguousarray(col_idx, np.int32)
        values = np.ascontiguousarray(values, np.float64)
        self.dtype = np.dtype(dtype)
        self.n = int(n)
        self.fmt = fmt
        self.h = C.c_void_p()
        self._lent = []
        o = _make_opts(opts)
        a = AmgOpts(C.sizeof(AmgOpts), theta, max_levels, coarse_rows, sweeps, coarse_sweeps)
        fmt_id = FORMATS[fmt] if isinstance(fmt, str) else fmt
        head = (C.byref(self.h), fmt_id, F64 if self.dtype == np.float64 else F32, C.c_long(n), _p(row_ptr), _p(col_idx), _p(values),
                C.byref(a))
        with_ = getattr(self, "_prolongator", None)                  # set by Amg.build alone
        if with_ is None:
            _check(lib().spmv_mi355x_amg_create(*head, C.byref(o)))
        else:
            near_null, filtered = with_
            if near_null is not None:
                near_null = np.ascontiguousarray(near_null, np.float64)
                if near_null.shape != (self.n,):
                    raise ValueError(f"near_null must have {self.n} values, got {near_null.shape}")
            po = AmgProlongatorOpts(C.sizeof(AmgProlongatorOpts), int(filtered), None if near_null is None else near_null.ctypes.data)
            _check(lib().spmv_mi355x_amg_create_with(*head, C.byref(po), C.byref(o)))
        self.mem_footprint = lib().spmv_mi355x_amg_mem_footprint(self.h)
        self.levels = self.info()["levels"]
        self.A = self.level_matrices(0)[0] if self.levels else None

    @classmethod
    def build(cls, row_ptr, col_idx, values, n, near_null=None, filtered=False, fmt="sell_c_sigma", dtype=np.float64, **kw):
        """An Amg through spmv_mi355x_amg_create_with: near_null = n fp64 values that the tentative prolongator carries instead of the
        constant (None: the constant), filtered = True smooths the prolongator with the filtered operator A_F. The other arguments
        are __init__'s (theta, max_levels, ..., **opts)."""
        self = cls.__new__(cls)
        self._prolongator = (near_null, filtered)
        self.__init__(row_ptr, col_idx, values, n, fmt, dtype, **kw)
        return self

    def prolongator_info(self):
        """dict of spmv_mi355x_amg_prolongator_stats, the per-level arrays cut to `levels` entries"""
        s = AmgProlongatorStats()
        s.struct_size = C.sizeof(AmgProlongatorStats)
        _check(lib().spmv_mi355x_amg_prolongator_info(self.h, C.byref(s)))
        out = {}
        for k, _ in AmgProlongatorStats._fields_:
            if k != "struct_size":
                v = getattr(s, k)
                out[k] = list(v)[:self.levels] if hasattr(v, "__len__") else v
        return out

    def near_null(self, level):
        """b_l, the near-null vector of level `level` (fp64); empty where none was given"""
        info = self.info()
        if not 0 <= level < info["levels"]:
            raise IndexError(f"level {level} of {info['levels']}")
        out = np.zeros(max(info["rows"][level], 1))
        _check(lib().spmv_mi355x_amg_near_null(self.h, C.c_int(level), _p(out)))
        return out[:info["rows"][level] if self.prolongator_info()["has_near_null"] else 0]

    def info(self):
        """dict of spmv_mi355x_amg_stats: the per-level arrays cut to `levels` entries, coarse_kind also as coarse ("dense",
        "sweeps", "sweeps after a failed pivot")"""
        s = AmgStats()
        s.struct_size = C.sizeof(AmgStats)
        _check(lib().spmv_mi355x_amg_info(self.h, C.byref(s)))
        out = {}
        for k, t in AmgStats._fields_:
            if k != "struct_size":
                v = getattr(s, k)
                out[k] = list(v)[:s.levels] if hasattr(v, "__len__") else v
        out["coarse"] = AMG_COARSE_KINDS[s.coarse_kind]
        return out

    def level_matrices(self, level):
        """(A_l, P_l, R_l) as Matrix objects over borrowed handles; P and R are None on the last level"""
        ptrs = [C.c_void_p(), C.c_void_p(), C.c_void_p()]
        _check(lib().spmv_mi355x_amg_level_matrices(self.h, C.c_int(level), *[C.byref(q) for q in ptrs]))
        out = tuple(Matrix(None, None, None, 0, 0, self.fmt, self.dtype, _handle=q, _borrowed=True) if q else None for q in ptrs)
        self._lent.extend(M for M in out if M is not None)
        return out

    def aggregates(self, level):
        """the aggregate of every row of level `level` (int32); empty where the level was not coarsened"""
        info = self.info()
        if not 0 <= level < info["levels"]:
            raise IndexError(f"level {level} of {info['levels']}")
        out = np.full(max(info["rows"][level], 1), -1, np.int32)
        _check(lib().spmv_mi355x_amg_aggregates(self.h, C.c_int(level), _p(out)))
        return out[:info["rows"][level] if info["mis_rounds"][level] else 0]

    def level_csr(self, level, which="A"):
        """(row_ptr, col_idx, values) in fp64 of A_l (which = "A") or P_l ("P"): what the handles were built from; "AF": the filtered
        operator of a coarsened level of a hierarchy built with filtered = True"""
        info = self.info()
        if not 0 <= level < info["levels"]:
            raise IndexError(f"level {level} of {info['levels']}")
        nnz = self.prolongator_info()["nnz_filtered"][level] if which == "AF" else info["nnz_p" if which == "P" else "nnz"][level]
        rp = np.zeros(info["rows"][level] + 1, np.int32)
        ci, va = np.zeros(max(nnz, 1), np.int32), np.zeros(max(nnz, 1))
        _check(lib().spmv_mi355x_amg_level_csr(self.h, C.c_int(level), C.c_int({"A": AMG_A, "P": AMG_P, "AF": AMG_AF}[which]), _p(rp), _p(ci),
                                               _p(va)))
        return rp, ci[:nnz], va[:nnz]

    def apply(self, v):
        """one cycle M^-1 v for a host vector of n values (spmv_mi355x_amg_apply; blocking)"""
        v = np.ascontiguousarray(v, self.dtype)
        if v.shape != (self.n,):
            raise ValueError(f"v must have {self.n} values, got {v.shape}")
        out = np.full(max(self.n, 1), np.nan, self.dtype)
        _check(lib().spmv_mi355x_amg_apply(self.h, _p(v), _p(out)))
        return out[:self.n]

    def apply_device(self, in_ptr, out_ptr, stream=None):
        """The same on device pointers (in_ptr == out_ptr: in place), enqueued on `stream` (spmv_mi355x_amg_apply_device_async)"""
        _check(lib().spmv_mi355x_amg_apply_device_async(self.h, C.c_void_p(in_ptr), C.c_void_p(out_ptr), C.c_void_p(stream or 0)))

    def apply_multi(self, V):
        """one cycle M^-1 V for the k columns of a host block of shape (n, k) (spmv_mi355x_amg_apply_multi; blocking): column j holds
        the bits of apply(V[:, j]) on a deterministic layout"""
        V = np.ascontiguousarray(V, self.dtype)
        if V.ndim != 2 or V.shape[0] != self.n or V.shape[1] < 1:
            raise ValueError(f"V must have shape ({self.n}, k) with k >= 1, got {V.shape}")
        out = np.zeros(V.shape, self.dtype)
        _check(lib().spmv_mi355x_amg_apply_multi(self.h, V.shape[1], _p(V), _p(out)))
        return out

    def apply_multi_device(self, k, in_ptr, ldin, out_ptr, ldout, stream=None):
        """The same on device blocks, row i at ptr + i * ld values (in_ptr == out_ptr with ldin == ldout: in place), enqueued on
        `stream` (spmv_mi355x_amg_apply_multi_device_async)"""
        _check(lib().spmv_mi355x_amg_apply_multi_device_async(self.h, k, in_ptr, ldin, out_ptr, ldout, stream or 0))

    def apply_multi_plan(self, k):
        """(matrix passes, launches) of one k-column cycle (spmv_mi355x_amg_apply_multi_plan; touches no device)"""
        passes, launches = C.c_long(0), C.c_long(0)
        _check(lib().spmv_mi355x_amg_apply_multi_plan(self.h, k, C.byref(passes), C.byref(launches)))
        return passes.value, launches.value

    def set_fold(self, rows):
        """rows > 0: the levels from the first one with at most `rows` rows on run as one launch of one workgroup per apply
        (spmv_mi355x_amg_set_fold; blocking); 0, the state after creation, turns the fold off"""
        _check(lib().spmv_mi355x_amg_set_fold(self.h, int(rows)))
        self.mem_footprint = lib().spmv_mi355x_amg_mem_footprint(self.h)

    @property
    def fold_rows(self):
        return self.fold_info()["fold_rows"]

    def fold_info(self):
        """dict of spmv_mi355x_amg_fold_stats, lanes_per_row cut to `levels` entries; first_level == levels: nothing folds"""
        s = AmgFoldStats()
        s.struct_size = C.sizeof(AmgFoldStats)
        _check(lib().spmv_mi355x_amg_fold_info(self.h, C.byref(s)))
        out = {k: getattr(s, k) for k, _ in AmgFoldStats._fields_ if k != "struct_size"}
        out["lanes_per_row"] = list(s.lanes_per_row)[:self.levels]
        return out

    def apply_level(self, level, v):
        """cycle(level, v) for a host vector of rows[level] values under the current fold setting (blocking)"""
        import torch
        rows = self.info()["rows"]
        if not 0 <= level < len(rows):
            raise IndexError(f"level {level} of {len(rows)}")
        v = np.ascontiguousarray(v, self.dtype)
        if v.shape != (rows[level],):
            raise ValueError(f"v must have {rows[level]} values, got {v.shape}")
        t = torch.from_numpy(v).cuda()
        u = torch.empty_like(t)
        self.apply_level_device(level, t.data_ptr(), u.data_ptr())
        torch.cuda.synchronize()
        return u.cpu().numpy()

    def apply_level_device(self, level, in_ptr, out_ptr, stream=None):
        """The same on device pointers (in_ptr == out_ptr: in place), enqueued on `stream` (spmv_mi355x_amg_apply_level_device_async)"""
        _check(lib().spmv_mi355x_amg_apply_level_device_async(self.h, C.c_int(level), C.c_void_p(in_ptr), C.c_void_p(out_ptr),
                                                              C.c_void_p(stream or 0)))

    def update_values_prepare(self):
        """once, before the first update_values: keeps the SpGEMM plans, the aggregates and the value arrays of every level on the
        device (spmv_mi355x_amg_update_values_prepare)"""
        _check(lib().spmv_mi355x_amg_update_values_prepare(self.h))

    def update_values(self, values):
        """new values of A in the entry order of the CSR given at creation: the aggregates and every pattern stay, the numbers of
        every level are recomputed on the device (spmv_mi355x_amg_update_values; blocking)"""
        values = np.ascontiguousarray(values, np.float64)
        nnz = self.info()["nnz"][0] if self.levels else 0
        if values.shape != (nnz,):
            raise ValueError(f"values must have {nnz} entries, got {values.shape}")
        _check(lib().spmv_mi355x_amg_update_values(self.h, _p(values)))

    def update_values_device(self, ptr, stream=0):
        """The same from nnz(A) fp64 values on the device, ordered on `stream`; blocking (spmv_mi355x_amg_update_values_device)"""
        _check(lib().spmv_mi355x_amg_update_values_device(self.h, C.c_void_p(ptr), C.c_void_p(stream or 0)))

    def update_values_state(self):
        """0 = cannot be updated (last_error says why), 1 = update_values_prepare is missing, 2 = ready, 3 = the last update failed"""
        return lib().spmv_mi355x_amg_update_values_state(self.h)

    def update_info(self):
        """dict of spmv_mi355x_amg_update_stats"""
        s = AmgUpdateStats()
        s.struct_size = C.sizeof(AmgUpdateStats)
        _check(lib().spmv_mi355x_amg_update_info(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in AmgUpdateStats._fields_ if k != "struct_size"}

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            for M in self._lent:
                M.close()
            self._lent = []
            lib().spmv_mi355x_amg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SpgemmStats(C.Structure):
    """spmv_mi355x_spgemm_stats (include/spmv_mi355x.h "SpGEMM")"""
    _fields_ = [("struct_size", C.c_uint), ("m", C.c_long), ("k", C.c_long), ("n", C.c_long), ("nnz_a", C.c_long),
                ("nnz_b", C.c_long), ("nnz_c", C.c_long), ("products", C.c_long), ("max_row_products", C.c_long),
                ("max_row_c", C.c_long), ("symbolic_bin_rows", C.c_long * 7), ("numeric_bin_rows", C.c_long * 7),
                ("symbolic_probes", C.c_long), ("symbolic_seconds", C.c_double), ("multiply_seconds", C.c_double),
                ("device_bytes", C.c_double)]


class SpGemm:
    """The plan of C = A B for A m x k and B k x n, int32 CSR (include/spmv_mi355x.h "SpGEMM"): the pattern of C is found once, on the
    GPU, here; multiply(a_values, b_values) computes C's fp64 values for one set of A's and B's values, in the entry order of
    (row_ptr, col_idx), bit for bit the sequential fma loop of the header. The plan holds patterns, never values."""

    def __init__(self, a_row_ptr, a_col_idx, m, k, b_row_ptr, b_col_idx, n, device=-1):
        a_rp = np.ascontiguousarray(a_row_ptr, np.int32)
        a_ci = np.ascontiguousarray(a_col_idx, np.int32)
        b_rp = np.ascontiguousarray(b_row_ptr, np.int32)
        b_ci = np.ascontiguousarray(b_col_idx, np.int32)
        self.h = C.c_void_p()
        _check(lib().spmv_mi355x_spgemm_create(C.byref(self.h), C.c_int(device), C.c_long(m), C.c_long(k), C.c_long(n), _p(a_rp),
                                               _p(a_ci), _p(b_rp), _p(b_ci)))
        st = self.info()
        self.shape = (st["m"], st["n"])
        self.nnz, self.nnz_a, self.nnz_b = st["nnz_c"], st["nnz_a"], st["nnz_b"]
        self.row_ptr = np.zeros(st["m"] + 1, np.int32)
        self.col_idx = np.zeros(self.nnz, np.int32)
        _check(lib().spmv_mi355x_spgemm_pattern(self.h, _p(self.row_ptr), _p(self.col_idx) if self.nnz else None))
        for a in (self.row_ptr, self.col_idx):
            a.setflags(write=False)

    def info(self):
        """dict of spmv_mi355x_spgemm_stats: m, k, n, nnz_a, nnz_b, nnz_c, products, max_row_products, max_row_c, symbolic_bin_rows,
        numeric_bin_rows (lists, one count per bin of csrc/spgemm.hpp), symbolic_probes, symbolic_seconds, multiply_seconds,
        device_bytes"""
        st = SpgemmStats()
        st.struct_size = C.sizeof(SpgemmStats)
        _check(lib().spmv_mi355x_spgemm_info(self.h, C.byref(st)))
        out = {}
        for name, ctype in SpgemmStats._fields_[1:]:
            v = getattr(st, name)
            out[name] = list(v) if hasattr(v, "__len__") else v
        return out

    def multiply(self, a_values, b_values):
        """C's fp64 values in C's entry order for these values of A and B (spmv_mi355x_spgemm_multiply; blocking)"""
        a = np.ascontiguousarray(a_values, np.float64)
        b = np.ascontiguousarray(b_values, np.float64)
        if a.shape != (self.nnz_a,) or b.shape != (self.nnz_b,):
            raise ValueError(f"a_values and b_values must have {self.nnz_a} and {self.nnz_b} entries, got {a.shape} and {b.shape}")
        out = np.full(max(self.nnz, 1), np.nan)
        _check(lib().spmv_mi355x_spgemm_multiply(self.h, _p(a), _p(b), _p(out)))
        return out[:self.nnz]

    def multiply_device(self, a_ptr, b_ptr, c_ptr, stream=0):
        """The same on device pointers to nnz_a, nnz_b and nnz fp64 values, enqueued on `stream`
        (spmv_mi355x_spgemm_multiply_device_async); c_ptr is what Matrix.update_values_device of a handle of C takes"""
        _check(lib().spmv_mi355x_spgemm_multiply_device_async(self.h, C.c_void_p(a_ptr), C.c_void_p(b_ptr), C.c_void_p(c_ptr),
                                                              C.c_void_p(stream or 0)))

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            lib().spmv_mi355x_spgemm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def spgemm(A, B, device=-1):
    """(row_ptr, col_idx, values) of C = A B for A = (row_ptr, col_idx, values, m, k) and B = (row_ptr, col_idx, values, k, n):
    one plan, one multiply"""
    a_rp, a_ci, a_va, m, k = A
    b_rp, b_ci, b_va, kb, n = B
    if k != kb:
        raise ValueError(f"A is {m} x {k} and B is {kb} x {n}")
    P = SpGemm(a_rp, a_ci, m, k, b_rp, b_ci, n, device)
    try:
        return P.row_ptr, P.col_idx, P.multiply(a_va, b_va)
    finally:
        P.close()


def _tri_precond(precond, m, dtype):
    """the TriPrecond of precond = (first, scale, second), and the scale array it points into (to be kept alive)"""
    first, scale, second = precond
    for T in (first, second):
        if T is not None and not isinstance(T, TriangularSolve):
            raise ValueError("precond = (first, scale, second): first and second are TriangularSolve handles or None")
    if scale is not None:
        scale = np.ascontiguousarray(scale, dtype)
        if scale.shape != (m,):
            raise ValueError(f"the scale of precond must have {m} values, got {scale.shape}")
    M = TriPrecond(C.sizeof(TriPrecond), None if first is None else first.h, None if scale is None else _p(scale),
                   None if second is None else second.h)
    return M, scale


class SolverInfo(C.Structure):
    """spmv_mi355x_solver_info (include/spmv_mi355x.h)"""
    _fields_ = [("struct_size", C.c_uint), ("iterations", C.c_long), ("error", C.c_double), ("error_best", C.c_double),
                ("eps", C.c_double), ("eps_counter", C.c_double), ("restarts", C.c_long), ("spmv_calls", C.c_long),
                ("seconds", C.c_double)]


class LsqInfo(C.Structure):
    """spmv_mi355x_lsq_info (include/spmv_mi355x.h)"""
    _fields_ = [("struct_size", C.c_uint), ("iterations", C.c_long), ("stop", C.c_int), ("rnorm", C.c_double), ("arnorm", C.c_double),
                ("arnorm0", C.c_double), ("xnorm", C.c_double), ("spmv_calls", C.c_long), ("seconds", C.c_double)]


class MinresInfo(C.Structure):
    """spmv_mi355x_minres_info (include/spmv_mi355x.h)"""
    _fields_ = [("struct_size", C.c_uint), ("iterations", C.c_long), ("stop", C.c_int), ("rnorm", C.c_double), ("rnorm0", C.c_double),
                ("prnorm", C.c_double), ("prnorm0", C.c_double), ("xnorm", C.c_double), ("spmv_calls", C.c_long),
                ("seconds", C.c_double)]


class GmresInfo(C.Structure):
    """spmv_mi355x_gmres_info (include/spmv_mi355x.h)"""
    _fields_ = [("struct_size", C.c_uint), ("iterations", C.c_long), ("stop", C.c_int), ("restarts", C.c_long), ("rnorm", C.c_double),
                ("rnorm0", C.c_double), ("prnorm", C.c_double), ("xnorm", C.c_double), ("spmv_calls", C.c_long),
                ("seconds", C.c_double)]


class PcgTriInfo(C.Structure):
    """spmv_mi355x_pcg_tri_info (include/spmv_mi355x.h)"""
    _fields_ = [("struct_size", C.c_uint), ("iterations", C.c_long), ("stop", C.c_int), ("rnorm", C.c_double), ("rnorm0", C.c_double),
                ("prnorm", C.c_double), ("xnorm", C.c_double), ("spmv_calls", C.c_long), ("seconds", C.c_double)]


class TriPrecond(C.Structure):
    """spmv_mi355x_tri_precond (include/spmv_mi355x.h)"""
    _fields_ = [("struct_size", C.c_uint), ("first", C.c_void_p), ("scale_host", C.c_void_p), ("second", C.c_void_p)]


SPMV_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)
ALLREDUCE_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int)


class DistOps(C.Structure):
    """spmv_mi355x_dist_ops (include/spmv_mi355x.h)"""
    _fields_ = [("struct_size", C.c_uint), ("row_offset", C.c_long), ("spmv", SPMV_CB), ("allreduce_sum", ALLREDUCE_CB),
                ("reduce_buf_dev", C.c_void_p), ("ctx", C.c_void_p)]


def solve_distributed(method, ops, dtype, m_local, row_ptr, col_idx, values, b, max_iterations, history=True):
    """spmv_mi355x_pcg_dist / spmv_mi355x_pbicgstab_dist: returns the same dict as Matrix.pcg for the LOCAL slice of x."""
    dtype = np.dtype(dtype)
    row_ptr = np.ascontiguousarray(row_ptr, np.int32)
    col_idx = np.ascontiguousarray(col_idx, np.int32)
    values = np.ascontiguousarray(values, np.float64)
    b = np.ascontiguousarray(b, dtype)
    x = np.zeros(max(m_local, 1), dtype)
    hist = np.zeros((max(max_iterations, 1), 3), np.float64) if history else None
    info = SolverInfo()
    info.struct_size = C.sizeof(SolverInfo)
    fn = lib().spmv_mi355x_pcg_dist if method == "pcg" else lib().spmv_mi355x_pbicgstab_dist
    _check(fn(C.byref(ops), F64 if dtype == np.float64 else F32, C.c_long(m_local), _p(row_ptr), _p(col_idx), _p(values),
              _p(b), _p(x), C.c_long(max_iterations), _p(hist) if history else None, C.byref(info)))
    out = {k: getattr(info, k) for k, _ in SolverInfo._fields_ if k != "struct_size"}
    out["x"] = x[:m_local]
    out["history"] = hist[:info.iterations] if history else None
    return out


class PartitionedMatrix:
    """One matrix cut into nnz-balanced row blocks over several GPUs of one node behind ONE handle
    (spmv_mi355x_create_partitioned): what the reference's single-process driver would hold as its Matrix_Format."""

    def __init__(self, row_ptr, col_idx, values, m, n, nparts, fmt="sell_c_sigma", dtype=np.float64, devices=None, exchange=0, **opts):
        row_ptr = np.ascontiguousarray(row_ptr, np.int32)
        col_idx = np.ascontiguousarray(col_idx, np.int32)
        values = np.ascontiguousarray(values, np.float64)
        self.dtype = np.dtype(dtype)
        o = Opts()
        o.struct_size = C.sizeof(Opts)
        o.device = -1
        for k, v in opts.items():
            if not hasattr(o, k):
                raise TypeError(f"unknown option {k}")
            setattr(o, k, v)
        dev = None if devices is None else np.ascontiguousarray(devices, np.int32)
        self.h = C.c_void_p()
        fmt_id = FORMATS[fmt] if isinstance(fmt, str) else fmt
        _check(lib().spmv_mi355x_create_partitioned(C.byref(self.h), C.c_int(nparts), None if dev is None else _p(dev), C.c_int(exchange),
                                                    fmt_id, F64 if self.dtype == np.float64 else F32, C.c_long(m), C.c_long(n),
                                                    C.c_long(len(col_idx)), _p(row_ptr), _p(col_idx), _p(values), C.byref(o)))
        L = lib()
        self.m, self.n, self.nparts = m, n, L.spmv_mi355x_partitioned_parts(self.h)
        self.format_name = L.spmv_mi355x_partitioned_format_name(self.h).decode()
        self.exchange = L.spmv_mi355x_partitioned_exchange(self.h).decode()
        self.mem_footprint = L.spmv_mi355x_partitioned_mem_footprint(self.h)
        off = np.zeros(self.nparts + 1, np.int64)
        _check(L.spmv_mi355x_partitioned_offsets(self.h, _p(off)))
        self.offsets = off

    def spmv(self, x, always_copy=True):
        x = np.ascontiguousarray(x, self.dtype)
        assert x.shape[0] == self.n
        y = np.ones(self.m + 64, self.dtype)
        lib().spmv_mi355x_partitioned_set_always_copy(self.h, 1 if always_copy else 0)
        _check(lib().spmv_mi355x_spmv_partitioned(self.h, _p(x), _p(y)))
        return y[:self.m].copy()

    def time(self, iters):
        ms = C.c_double()
        _check(lib().spmv_mi355x_time_partitioned(self.h, C.c_int(iters), C.byref(ms)))
        return ms.value

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            lib().spmv_mi355x_destroy_partitioned(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Matrix:
    """One converted matrix on one GPU = the reference's `struct Matrix_Format` instance. Matrix(..., transpose=1) holds the
    transpose of the CSR it is given (include/spmv_mi355x.h "transposed handles"): m and n are then those of the transpose, and
    `transposed` is 1."""

    def __init__(self, row_ptr, col_idx, values, m, n, fmt="csr_vector", dtype=np.float64, _handle=None, _borrowed=False, **opts):
        self._borrowed = _borrowed                     # Fsai.G / Fsai.Gt: the handle belongs to another object and is never destroyed here
        if _handle is not None:                        # CsrStream.finish(), Fsai: the handle exists already
            self.dtype = np.dtype(dtype)
            self.h = _handle
            self._describe()
            return
        row_ptr = np.ascontiguousarray(row_ptr, np.int32)
        col_idx = np.ascontiguousarray(col_idx, np.int32)
        values = np.ascontiguousarray(values, np.float64)
        self.dtype = np.dtype(dtype)
        o = Opts()
        o.struct_size = C.sizeof(Opts)
        o.device = -1
        for k, v in opts.items():
            if not hasattr(o, k):
                raise TypeError(f"unknown option {k}")
            setattr(o, k, v)
        self.h = C.c_void_p()
        fmt_id = FORMATS[fmt] if isinstance(fmt, str) else fmt
        _check(lib().spmv_mi355x_create(C.byref(self.h), fmt_id, F64 if self.dtype == np.float64 else F32,
                                        C.c_long(m), C.c_long(n), C.c_long(len(col_idx)),
                                        _p(row_ptr), _p(col_idx), _p(values), C.byref(o)))
        self._describe()

    def _describe(self):
        L = lib()
        self.m = L.spmv_mi355x_rows(self.h)
        self.n = L.spmv_mi355x_cols(self.h)
        self.nnz = L.spmv_mi355x_nnz(self.h)
        self.format_name = L.spmv_mi355x_format_name(self.h).decode()
        self.mem_footprint = L.spmv_mi355x_mem_footprint(self.h)
        self.csr_mem_footprint = L.spmv_mi355x_csr_mem_footprint(self.h)
        # what the matrix values are stored as (opts.value_storage); self.dtype stays the precision of x and y
        self.value_dtype = np.dtype(np.float32 if L.spmv_mi355x_value_storage(self.h) == F32 else np.float64)
        self.transposed = L.spmv_mi355x_transposed(self.h)

    # Matrix_Format::spmv(x, y) on host buffers; y gets the driver's +64 slack and 1.0 canary (bench_spmv.cpp:606-609)
    def spmv(self, x, always_copy=True):
        x = np.ascontiguousarray(x, self.dtype)
        assert x.shape[0] == self.n
        y = np.ones(self.m + 64, self.dtype)
        lib().spmv_mi355x_set_always_copy(self.h, 1 if always_copy else 0)
        _check(lib().spmv_mi355x_spmv(self.h, _p(x), _p(y)))
        return y[:self.m].copy()

    def spmv_raw(self, x, y):
        """Exact reference call shape: caller-owned buffers, reference caching semantics."""
        _check(lib().spmv_mi355x_spmv(self.h, _p(x), _p(y)))

    def set_always_copy(self, on):
        lib().spmv_mi355x_set_always_copy(self.h, 1 if on else 0)

    def spmv_device(self, x_ptr, y_ptr, beta=0, stream=0):
        _check(lib().spmv_mi355x_spmv_device_async(self.h, C.c_void_p(x_ptr), C.c_void_p(y_ptr), C.c_int(beta),
                                                   C.c_void_p(stream)))

    def time_device(self, x_ptr, y_ptr, iters, stream=0):
        ms = C.c_double()
        _check(lib().spmv_mi355x_time_device(self.h, C.c_void_p(x_ptr), C.c_void_p(y_ptr), C.c_int(iters),
                                             C.c_void_p(stream), C.byref(ms)))
        return ms.value

    def spmm(self, X):
        """Y = A X for a host array X of shape (cols, k): returns Y of shape (rows, k) (spmv_mi355x_spmm; one pass over the matrix per
        8 columns on the SELL delta layout, per spmm_plan(k)[1] columns on the LDS-window layout)."""
        X = np.ascontiguousarray(X, self.dtype)
        if X.ndim != 2 or X.shape[0] != self.n:
            raise ValueError(f"X must have shape ({self.n}, k), got {X.shape}")
        k = X.shape[1]
        Y = np.zeros((self.m, k), self.dtype)
        _check(lib().spmv_mi355x_spmm(self.h, C.c_int(k), _p(X), _p(Y)))
        return Y

    def spmm_device(self, k, x_ptr, ldx, y_ptr, ldy, beta=0, stream=0):
        """Y = A X (beta 0) / Y += A X (beta 1) on device pointers: X has cols rows of k values ldx apart, Y rows rows ldy apart (in
        values); enqueued on `stream` (spmv_mi355x_spmm_device_async)."""
        _check(lib().spmv_mi355x_spmm_device_async(self.h, C.c_int(k), C.c_void_p(x_ptr), C.c_long(ldx), C.c_void_p(y_ptr), C.c_long(ldy),
                                                   C.c_int(beta), C.c_void_p(stream)))

    def spmm_plan(self, k):
        """(passes over the matrix arrays, most columns one pass serves) of an spmm with k columns on this handle
        (spmv_mi355x_spmm_plan): (k, 1) = served column by column, (0, 0) = a handle without entries."""
        passes, cols = C.c_int(), C.c_int()
        _check(lib().spmv_mi355x_spmm_plan(self.h, C.c_int(k), C.byref(passes), C.byref(cols)))
        return passes.value, cols.value

    def time_spmm_device(self, k, x_ptr, ldx, y_ptr, ldy, iters, stream=0):
        """ms per spmm of `iters` back-to-back launches, timed with HIP events on `stream` (spmv_mi355x_time_spmm_device)."""
        ms = C.c_double()
        _check(lib().spmv_mi355x_time_spmm_device(self.h, C.c_int(k), C.c_void_p(x_ptr), C.c_long(ldx), C.c_void_p(y_ptr), C.c_long(ldy),
                                                  C.c_int(iters), C.c_void_p(stream), C.byref(ms)))
        return ms.value

    # ---- new values for an existing handle (include/spmv_mi355x.h): same pattern, new numbers
    def update_values_prepare(self, row_ptr):
        """Once per handle before the first update: the LOCAL row pointer the handle was built from (rows + 1 entries from 0)."""
        row_ptr = np.ascontiguousarray(row_ptr, np.int32)
        if row_ptr.shape != (self.m + 1,):
            raise ValueError(f"row_ptr must have {self.m + 1} entries, got {row_ptr.shape}")
        _check(lib().spmv_mi355x_update_values_prepare(self.h, _p(row_ptr)))

    def update_values_prepare_transposed(self, row_ptr, col_idx, m, n):
        """Once per handle created with transpose=1, before its first update: the pattern of A (m x n) as the handle was created from.
        From then on update_values takes update_values_count() values in A's entry order (spmv_mi355x_update_values_prepare_transposed)."""
        row_ptr = np.ascontiguousarray(row_ptr, np.int32)
        col_idx = np.ascontiguousarray(col_idx, np.int32)
        if row_ptr.shape != (m + 1,) or col_idx.shape != (int(row_ptr[-1]),):
            raise ValueError(f"row_ptr must have {m + 1} entries and col_idx row_ptr[m], got {row_ptr.shape} and {col_idx.shape}")
        _check(lib().spmv_mi355x_update_values_prepare_transposed(self.h, C.c_long(m), C.c_long(n), _p(row_ptr), _p(col_idx)))

    def update_values_count(self):
        """The values an update of this handle reads: nnz, and the nnz of A once update_values_prepare_transposed has run."""
        return lib().spmv_mi355x_update_values_count(self.h)

    def update_values(self, values):
        """Replace the stored values by update_values_count() fp64 values in the order of the handle's local CSR — of the CSR of A
        for a prepared transposed handle (spmv_mi355x_update_values); what create() derives from the values (format_name,
        mem_footprint) is refreshed."""
        values = np.ascontiguousarray(values, np.float64)
        count = self.update_values_count()
        if values.shape != (count,):
            raise ValueError(f"values must have {count} entries, got {values.shape}")
        _check(lib().spmv_mi355x_update_values(self.h, _p(values)))
        self._describe()

    def update_values_device(self, ptr, stream=0):
        """The same from update_values_count() fp64 values resident on the handle's device, ordered on `stream`; blocking."""
        _check(lib().spmv_mi355x_update_values_device(self.h, C.c_void_p(ptr), C.c_void_p(stream)))
        self._describe()

    def update_values_state(self):
        """0 = this handle cannot be updated (spmv_mi355x_last_error says why), 1 = prepare is still missing, 2 = ready."""
        return lib().spmv_mi355x_update_values_state(self.h)

    def kernel_info(self):
        name = C.create_string_buffer(128)
        grid = C.c_long()
        block = C.c_int()
        _check(lib().spmv_mi355x_kernel_info(self.h, name, C.c_long(128), C.byref(grid), C.byref(block)))
        return dict(name=name.value.decode(), grid=grid.value, block=block.value)

    def x_device(self):
        return lib().spmv_mi355x_x_device(self.h)

    def y_device(self):
        return lib().spmv_mi355x_y_device(self.h)

    def upload_x(self, x):
        x = np.ascontiguousarray(x, self.dtype)
        _check(lib().spmv_mi355x_upload_x(self.h, _p(x)))

    def output_vector(self, count=None):
        """An engine-placed device vector for this handle's SpMV to write (rows + 64 values by default)."""
        return OutputVector(self, self.m + 64 if count is None else count)

    def input_vector(self, count=None):
        """An engine-placed device vector for this handle's SpMV to READ as x (cols values by default); `.torch()` gives the zero-copy
        tensor a collective can write into."""
        return OutputVector(self, self.n if count is None else count, is_input=True)

    def upload_y(self, y):
        y = np.ascontiguousarray(y, self.dtype)
        assert y.shape[0] >= self.m
        _check(lib().spmv_mi355x_upload_y(self.h, _p(y)))

    def download_y(self):
        y = np.zeros(self.m, self.dtype)
        _check(lib().spmv_mi355x_download_y(self.h, _p(y)))
        return y

    def sell_layout(self):
        Cc, sig, ns, ne = C.c_long(), C.c_long(), C.c_long(), C.c_long()
        sp = C.POINTER(C.c_int64)()
        col = C.POINTER(C.c_int32)()
        val = C.POINTER(C.c_double)()
        ros = C.POINTER(C.c_int32)()
        _check(lib().spmv_mi355x_sell_layout(self.h, C.byref(Cc), C.byref(sig), C.byref(ns), C.byref(ne),
                                             C.byref(sp), C.byref(col), C.byref(val), C.byref(ros)))
        out = dict(C=Cc.value, sigma=sig.value, num_slices=ns.value, nnz_ext=ne.value,
                   slice_ptr=np.ctypeslib.as_array(sp, shape=(ns.value + 1,)).copy(),
                   col=np.ctypeslib.as_array(col, shape=(max(ne.value, 1),))[:ne.value].copy(),
                   val=np.ctypeslib.as_array(val, shape=(max(ne.value, 1),))[:ne.value].copy(),
                   row_of_sorted=np.ctypeslib.as_array(ros, shape=(max(self.m, 1),))[:self.m].copy())
        for p in (sp, col, val, ros):
            lib().spmv_mi355x_free(p)
        return out

    def place_arrays(self, x_ptr, y_ptr):
        """The search over the handle's matrix arrays (opts.placement = 3) for a caller's device vectors; y is overwritten."""
        _check(lib().spmv_mi355x_place_arrays(self.h, C.c_void_p(x_ptr), C.c_void_p(y_ptr)))

    def stored_array(self, name, dtype=np.uint8):
        """One stored array of the LDS-window SELL / column-blocked layout as it lies in device memory (include/spmv_mi355x.h)."""
        out, nb = C.c_void_p(), C.c_size_t()
        _check(lib().spmv_mi355x_stored_array(self.h, name.encode(), C.byref(out), C.byref(nb)))
        a = np.frombuffer(C.string_at(out.value, nb.value), dtype=np.uint8).copy().view(dtype) if nb.value else np.zeros(0, dtype)
        lib().spmv_mi355x_free(out)
        return a

    def merge_tiles(self):
        nt, ti = C.c_long(), C.c_long()
        co = C.POINTER(C.c_int32)()
        _check(lib().spmv_mi355x_merge_tiles(self.h, C.byref(nt), C.byref(ti), C.byref(co)))
        coords = np.ctypeslib.as_array(co, shape=(2 * (nt.value + 1),)).copy().reshape(-1, 2)
        lib().spmv_mi355x_free(co)
        return dict(num_tiles=nt.value, tile_items=ti.value, coords=coords)

    def _solve(self, fn, row_ptr, col_idx, values, b, max_iterations, history):
        row_ptr = np.ascontiguousarray(row_ptr, np.int32)
        col_idx = np.ascontiguousarray(col_idx, np.int32)
        values = np.ascontiguousarray(values, np.float64)
        b = np.ascontiguousarray(b, self.dtype)
        assert b.shape[0] == self.m and len(row_ptr) == self.m + 1
        x = np.zeros(max(self.n, 1), self.dtype)
        hist = np.zeros((max(max_iterations, 1), 3), np.float64) if history else None
        info = SolverInfo()
        info.struct_size = C.sizeof(SolverInfo)
        _check(fn(self.h, _p(row_ptr), _p(col_idx), _p(values), _p(b), _p(x), C.c_long(max_iterations),
                  _p(hist) if history else None, C.byref(info)))
        out = {k: getattr(info, k) for k, _ in SolverInfo._fields_ if k != "struct_size"}
        out["x"] = x[:self.n]
        out["history"] = hist[:info.iterations] if history else None
        return out

    def pcg(self, row_ptr, col_idx, values, b, max_iterations, history=True):
        """preconditioned_cg() of bench_cg.cpp:93-322 with every vector resident in HBM."""
        return self._solve(lib().spmv_mi355x_pcg, row_ptr, col_idx, values, b, max_iterations, history)

    def pbicgstab(self, row_ptr, col_idx, values, b, max_iterations, history=True):
        """preconditioned_bicgstab() of bench_bicg.cpp:149-459 with every vector resident in HBM."""
        return self._solve(lib().spmv_mi355x_pbicgstab, row_ptr, col_idx, values, b, max_iterations, history)

    def _solve_multi(self, fn, row_ptr, col_idx, values, B, max_iterations, history):
        row_ptr = np.ascontiguousarray(row_ptr, np.int32)
        col_idx = np.ascontiguousarray(col_idx, np.int32)
        values = np.ascontiguousarray(values, np.float64)
        B = np.ascontiguousarray(B, self.dtype)
        if B.ndim != 2 or B.shape[0] != self.m or B.shape[1] < 1:
            raise ValueError(f"B must have shape ({self.m}, k) with k >= 1, got {B.shape}")
        assert len(row_ptr) == self.m + 1
        k = B.shape[1]
        X = np.zeros((max(self.m, 1), k), self.dtype)
        hist = np.zeros(k * max(max_iterations, 1) * 3, np.float64) if history else None
        info = (SolverInfo * k)()
        info[0].struct_size = C.sizeof(SolverInfo)
        _check(fn(self.h, C.c_int(k), _p(row_ptr), _p(col_idx), _p(values), _p(B), _p(X), C.c_long(max_iterations),
                  _p(hist) if history else None, info))
        out = []
        for j in range(k):
            d = {f: getattr(info[j], f) for f, _ in SolverInfo._fields_ if f != "struct_size"}
            d["x"] = X[:self.n, j].copy()
            d["history"] = hist[j * 3 * max_iterations:(j + 1) * 3 * max_iterations].reshape(max_iterations, 3)[:d["iterations"]].copy() \
                if history else None
            out.append(d)
        return out

    def pcg_multi(self, row_ptr, col_idx, values, B, max_iterations, history=True):
        """Matrix.pcg for the k columns of B (shape (rows, k)) in one solve with one SpMM per iteration
        (spmv_mi355x_pcg_multi): a list of k dicts, element j bit-identical to pcg(B[:, j]) on a deterministic handle."""
        return self._solve_multi(lib().spmv_mi355x_pcg_multi, row_ptr, col_idx, values, B, max_iterations, history)

    def pbicgstab_multi(self, row_ptr, col_idx, values, B, max_iterations, history=True):
        """Matrix.pbicgstab for the k columns of B (spmv_mi355x_pbicgstab_multi), as pcg_multi."""
        return self._solve_multi(lib().spmv_mi355x_pbicgstab_multi, row_ptr, col_idx, values, B, max_iterations, history)

    def cgls(self, At, b, damp=0.0, tol=1e-12, max_iterations=1000, history=True):
        """min |A x - b|^2 + damp |x|^2 by CGLS over this handle (A) and `At`, a handle of its transpose (spmv_mi355x_cgls): a dict of
        the spmv_mi355x_lsq_info fields plus x (cols values) and history (rows (|r_{k+1}|, |s_{k+1}|), shape (iterations, 2), or None).
        The shape, precision and device of At are checked by the library."""
        b = np.ascontiguousarray(b, self.dtype)
        if b.shape != (self.m,):
            raise ValueError(f"b must have {self.m} values, got {b.shape}")
        x = np.zeros(max(self.n, 1), self.dtype)
        hist = np.zeros((max(max_iterations, 1), 2), np.float64) if history else None
        info = LsqInfo()
        info.struct_size = C.sizeof(LsqInfo)
        _check(lib().spmv_mi355x_cgls(self.h, At.h, _p(b), _p(x), damp, tol, max_iterations, _p(hist) if history else None,
                                      C.byref(info)))
        out = {k: getattr(info, k) for k, _ in LsqInfo._fields_ if k != "struct_size"}
        out["x"] = x[:self.n]
        out["history"] = hist[:info.iterations] if history else None
        return out

    def minres(self, b, shift=0.0, minv=None, tol=1e-12, max_iterations=1000, history=True):
        """(A - shift I) x = b by MINRES for a square symmetric matrix, indefinite included (spmv_mi355x_minres): a dict of the
        spmv_mi355x_minres_info fields plus x (rows values) and history (phibar after each iteration, shape (iterations,), or None).
        `minv`, when given, is the inverse of a diagonal preconditioner: rows values, every one finite and > 0 (checked by the library,
        like the shape of the handle)."""
        b = np.ascontiguousarray(b, self.dtype)
        if b.shape != (self.m,):
            raise ValueError(f"b must have {self.m} values, got {b.shape}")
        if minv is not None:
            minv = np.ascontiguousarray(minv, self.dtype)
            if minv.shape != (self.m,):
                raise ValueError(f"minv must have {self.m} values, got {minv.shape}")
        x = np.zeros(max(self.m, 1), self.dtype)
        hist = np.zeros(max(max_iterations, 1), np.float64) if history else None
        info = MinresInfo()
        info.struct_size = C.sizeof(MinresInfo)
        _check(lib().spmv_mi355x_minres(self.h, _p(b), _p(x), shift, None if minv is None else _p(minv), tol, max_iterations,
                                        _p(hist) if history else None, C.byref(info)))
        out = {k: getattr(info, k) for k, _ in MinresInfo._fields_ if k != "struct_size"}
        out["x"] = x[:self.m]
        out["history"] = hist[:info.iterations] if history else None
        return out

    def gmres(self, b, restart=30, minv=None, tol=1e-12, max_iterations=1000, history=True, precond=None):
        """A x = b by restarted GMRES(restart) for any square matrix (spmv_mi355x_gmres): a dict of the spmv_mi355x_gmres_info fields
        plus x (rows values) and history (|g| after each inner step, shape (iterations,), or None). `minv`, when given, is the inverse
        of a diagonal right preconditioner: rows values, every one finite and > 0 (checked by the library, like `restart` and the
        shape of the handle). `precond` = (first, scale, second) instead applies second^-1 (scale * (first^-1 v)) (spmv_mi355x_gmres_tri):
        first / second are TriangularSolve handles or None, scale an array of rows values or None."""
        b = np.ascontiguousarray(b, self.dtype)
        if b.shape != (self.m,):
            raise ValueError(f"b must have {self.m} values, got {b.shape}")
        if precond is not None and minv is not None:
            raise ValueError("minv and precond are two forms of the one right preconditioner: give one of them")
        if precond is not None:
            M, scale = _tri_precond(precond, self.m, self.dtype)
        if minv is not None:
            minv = np.ascontiguousarray(minv, self.dtype)
            if minv.shape != (self.m,):
                raise ValueError(f"minv must have {self.m} values, got {minv.shape}")
        x = np.zeros(max(self.m, 1), self.dtype)
        hist = np.zeros(max(max_iterations, 1), np.float64) if history else None
        info = GmresInfo()
        info.struct_size = C.sizeof(GmresInfo)
        if precond is not None:
            _check(lib().spmv_mi355x_gmres_tri(self.h, _p(b), _p(x), restart, C.byref(M), tol, max_iterations,
                                               _p(hist) if history else None, C.byref(info)))
        else:
            _check(lib().spmv_mi355x_gmres(self.h, _p(b), _p(x), restart, None if minv is None else _p(minv), tol, max_iterations,
                                           _p(hist) if history else None, C.byref(info)))
        out = {k: getattr(info, k) for k, _ in GmresInfo._fields_ if k != "struct_size"}
        out["x"] = x[:self.m]
        out["history"] = hist[:info.iterations] if history else None
        return out

    def pcg_tri(self, b, precond=None, tol=1e-12, max_iterations=1000, history=True):
        """A x = b by preconditioned CG for a square symmetric positive definite matrix (spmv_mi355x_pcg_tri): a dict of the
        spmv_mi355x_pcg_tri_info fields plus x (rows values) and history (|r| of the recurrence after each iteration, shape
        (iterations,), or None). `precond` = (first, scale, second) applies second^-1 (scale * (first^-1 v)) as M^-1: first / second
        are TriangularSolve handles or None, scale an array of rows values or None (sgs_precond builds the SGS of A); None is the
        plain CG. An Fsai object as `precond` applies its G^t (G v) instead (spmv_mi355x_pcg_fsai), an Amg object its V cycle
        (spmv_mi355x_pcg_amg)."""
        b = np.ascontiguousarray(b, self.dtype)
        if b.shape != (self.m,):
            raise ValueError(f"b must have {self.m} values, got {b.shape}")
        M = None
        if isinstance(precond, (Fsai, Amg)):
            x = np.zeros(max(self.m, 1), self.dtype)
            hist = np.zeros(max(max_iterations, 1), np.float64) if history else None
            info = PcgTriInfo()
            info.struct_size = C.sizeof(PcgTriInfo)
            solve = lib().spmv_mi355x_pcg_fsai if isinstance(precond, Fsai) else lib().spmv_mi355x_pcg_amg
            _check(solve(self.h, _p(b), _p(x), precond.h, tol, max_iterations, _p(hist) if history else None, C.byref(info)))
            out = {k: getattr(info, k) for k, _ in PcgTriInfo._fields_ if k != "struct_size"}
            out["x"] = x[:self.m]
            out["history"] = hist[:info.iterations] if history else None
            return out
        if precond is not None:
            M, scale = _tri_precond(precond, self.m, self.dtype)
        x = np.zeros(max(self.m, 1), self.dtype)
        hist = np.zeros(max(max_iterations, 1), np.float64) if history else None
        info = PcgTriInfo()
        info.struct_size = C.sizeof(PcgTriInfo)
        _check(lib().spmv_mi355x_pcg_tri(self.h, _p(b), _p(x), None if M is None else C.byref(M), tol, max_iterations,
                                         _p(hist) if history else None, C.byref(info)))
        out = {k: getattr(info, k) for k, _ in PcgTriInfo._fields_ if k != "struct_size"}
        out["x"] = x[:self.m]
        out["history"] = hist[:info.iterations] if history else None
        return out

    def pcg_tri_multi(self, B, precond=None, tol=1e-12, max_iterations=1000, history=True):
        """pcg_tri for the k columns of B (shape (rows, k)) in one solve with one SpMM per iteration (spmv_mi355x_pcg_tri_multi,
        _pcg_fsai_multi, _pcg_amg_multi): a list of k dicts shaped like pcg_tri's, element j bit-identical to pcg_tri(B[:, j], precond)
        on a deterministic handle; spmv_calls and seconds are the call's. `precond` is None, (None, scale, None), an Fsai or an Amg;
        one with a TriangularSolve part raises the library's refusal (there is no k-column triangular solve)."""
        B = np.ascontiguousarray(B, self.dtype)
        if B.ndim != 2 or B.shape[0] != self.m or B.shape[1] < 1:
            raise ValueError(f"B must have shape ({self.m}, k) with k >= 1, got {B.shape}")
        k = B.shape[1]
        X = np.zeros((max(self.m, 1), k), self.dtype)
        hist = np.zeros(k * max(max_iterations, 1), np.float64) if history else None
        infos = (PcgTriInfo * k)()
        for j in range(k):
            infos[j].struct_size = C.sizeof(PcgTriInfo)
        hp = _p(hist) if history else None
        if isinstance(precond, (Fsai, Amg)):
            solve = lib().spmv_mi355x_pcg_fsai_multi if isinstance(precond, Fsai) else lib().spmv_mi355x_pcg_amg_multi
            _check(solve(self.h, k, _p(B), _p(X), precond.h, tol, max_iterations, hp, infos))
        else:
            M = None
            if precond is not None:
                M, scale = _tri_precond(precond, self.m, self.dtype)
            _check(lib().spmv_mi355x_pcg_tri_multi(self.h, k, _p(B), _p(X), None if M is None else C.byref(M), tol, max_iterations, hp,
                                                   infos))
        out = []
        for j in range(k):
            d = {f: getattr(infos[j], f) for f, _ in PcgTriInfo._fields_ if f != "struct_size"}
            d["x"] = X[:self.m, j].copy()
            d["history"] = hist[j * max_iterations:j * max_iterations + d["iterations"]].copy() if history else None
            out.append(d)
        return out

    def pcg_trsm_multi(self, B, precond=None, tol=1e-12, max_iterations=1000, history=True):
        """pcg_tri for the k columns of B (shape (rows, k)) with ANY (first, scale, second) that pcg_tri takes, e.g. what sgs_precond
        returns: the triangular parts run as k-column solves (spmv_mi355x_pcg_trsm_multi). A list of k dicts shaped like pcg_tri's,
        element j bit-identical to pcg_tri(B[:, j], precond) on a deterministic handle; spmv_calls and seconds are the call's."""
        B = np.ascontiguousarray(B, self.dtype)
        if B.ndim != 2 or B.shape[0] != self.m or B.shape[1] < 1:
            raise ValueError(f"B must have shape ({self.m}, k) with k >= 1, got {B.shape}")
        k = B.shape[1]
        M = None
        if precond is not None:
            M, scale = _tri_precond(precond, self.m, self.dtype)
        X = np.zeros((max(self.m, 1), k), self.dtype)
        hist = np.zeros(k * max(max_iterations, 1), np.float64) if history else None
        infos = (PcgTriInfo * k)()
        for j in range(k):
            infos[j].struct_size = C.sizeof(PcgTriInfo)
        _check(lib().spmv_mi355x_pcg_trsm_multi(self.h, k, _p(B), _p(X), None if M is None else C.byref(M), tol, max_iterations,
                                                _p(hist) if history else None, infos))
        out = []
        for j in range(k):
            d = {f: getattr(infos[j], f) for f, _ in PcgTriInfo._fields_ if f != "struct_size"}
            d["x"] = X[:self.m, j].copy()
            d["history"] = hist[j * max_iterations:j * max_iterations + d["iterations"]].copy() if history else None
            out.append(d)
        return out

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            if not getattr(self, "_borrowed", False):
                lib().spmv_mi355x_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
