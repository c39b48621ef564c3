"""ctypes binding of the C ABI declared in include/pepsgpu.h (libpepsgpu.so, HIP/gfx950).

This is the Python-side stub a maintainer would write to bind the library; it contains no
arithmetic and no CPU fallback: if the shared library is missing, import fails loudly.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# PEPSGPU_LIB: another build of the same library (A/B measurements of kernel variants); there is no non-HIP implementation
LIB_PATH = os.environ.get("PEPSGPU_LIB") or os.path.join(_HERE, "lib", "libpepsgpu.so")

F32, F64 = 0, 1
C128 = 3          # complex float64 (TenElemT = QLTEN_Complex): every scalar / tensor output becomes complex128
LEFT, DOWN, RIGHT, UP = 0, 1, 2, 3
HORIZONTAL, VERTICAL = 0, 1
LEFTUP_TO_RIGHTDOWN, LEFTDOWN_TO_RIGHTUP = 0, 1   # basic.h:89-92 DIAGONAL_DIR
SVD_COMPRESS, VARIATION2SITE, VARIATION1SITE = 0, 1, 2   # CompressMPSScheme, bmps.h:31-35

_ERR = {1: ValueError, 2: RuntimeError, 3: RuntimeError, 4: IndexError, 5: RuntimeError}

SYMBOLS = [
    "pepsgpu_ctx_create", "pepsgpu_set_truncate_params", "pepsgpu_ctx_destroy", "pepsgpu_last_error", "pepsgpu_state_upload",
    "pepsgpu_walkers_set_configs", "pepsgpu_walkers_get_configs", "pepsgpu_n_walkers",
    "pepsgpu_grow_bmps_step", "pepsgpu_grow_full_bmps", "pepsgpu_grow_bmps_for_row", "pepsgpu_grow_bmps_for_col",
    "pepsgpu_shift_bmps_window", "pepsgpu_delete_inner_bmps", "pepsgpu_bmps_park", "pepsgpu_bmps_unpark", "pepsgpu_generate_bmps_approach",
    "pepsgpu_sweep_slice_exchange", "pepsgpu_sweep_slice_exchange_tab", "pepsgpu_sweep_slice_fullspace", "pepsgpu_sweep_slice_tnn3", "pepsgpu_diag_tnn3_table", "pepsgpu_nn_exchange_slice", "pepsgpu_nn_exchange_slice_tab", "pepsgpu_onsite_slice", "pepsgpu_nnn_exchange_slice", "pepsgpu_diag_nnn_slice_calls", "pepsgpu_nnn_hop_slice_fermion", "pepsgpu_diag_nnn_hop_slice_calls", "pepsgpu_diag_fermion_hop_cand", "pepsgpu_nn_pair_slice_fermion", "pepsgpu_diag_pair_slice_calls", "pepsgpu_diag_pair_cand", "pepsgpu_nn_hop_slice_fermion", "pepsgpu_diag_hop_slice_calls", "pepsgpu_sweep_slice_sector", "pepsgpu_diag_sector_slice_calls", "pepsgpu_diag_sector_cand", "pepsgpu_link_exchange_slice", "pepsgpu_diag_link_slice_calls", "pepsgpu_diag_link_cand", "pepsgpu_walker_create", "pepsgpu_walker_clone", "pepsgpu_walker_destroy", "pepsgpu_walker_info", "pepsgpu_walker_set_mpo", "pepsgpu_walker_set_mpo_excited", "pepsgpu_walker_trace_slice", "pepsgpu_diag_walker_slice_calls", "pepsgpu_walker_set_mpo_excited_pair", "pepsgpu_walker_pair_trace_slice", "pepsgpu_diag_walker_pair_slice_calls", "pepsgpu_diag_walker_pair_cand", "pepsgpu_walker_evolve",
    "pepsgpu_walker_evolve_step", "pepsgpu_walker_contract_row", "pepsgpu_walker_init_bten", "pepsgpu_walker_grow_bten_step",
    "pepsgpu_walker_shift_bten_window", "pepsgpu_walker_trace_with_bten", "pepsgpu_walker_clear_bten", "pepsgpu_walker_get_bmps_tensor",
    "pepsgpu_bmps_stack_size", "pepsgpu_get_bmps_tensor", "pepsgpu_init_bten", "pepsgpu_grow_full_bten",
    "pepsgpu_grow_bten_step", "pepsgpu_shift_bten_window", "pepsgpu_truncate_bten", "pepsgpu_bten_stack_size",
    "pepsgpu_trace", "pepsgpu_replace_nn_trace", "pepsgpu_replace_one_trace", "pepsgpu_trace_scaling", "pepsgpu_punch_hole",
    "pepsgpu_init_bten2", "pepsgpu_grow_full_bten2", "pepsgpu_grow_bten2_step", "pepsgpu_shift_bten2_window",
    "pepsgpu_bten2_stack_size", "pepsgpu_replace_nnn_trace", "pepsgpu_replace_tnn_trace",
    "pepsgpu_bten2_select_set", "pepsgpu_cfg_override_slice", "pepsgpu_replace_plaquette_trace",
    "pepsgpu_replace_sqrt5_trace",
    "pepsgpu_grad_reset", "pepsgpu_grad_accumulate", "pepsgpu_grad_accumulate_states", "pepsgpu_grad_read", "pepsgpu_grad_device_ptr", "pepsgpu_grad_allreduce", "pepsgpu_bcast_state",
    "pepsgpu_comm_unique_id", "pepsgpu_comm_init", "pepsgpu_comm_size", "pepsgpu_comm_rank", "pepsgpu_comm_destroy",
    "pepsgpu_allreduce",
    "pepsgpu_sr_begin", "pepsgpu_sr_append", "pepsgpu_sr_count", "pepsgpu_sr_sum", "pepsgpu_sr_matvec", "pepsgpu_sr_matvec_c128",
    "pepsgpu_sr_cg_solve", "pepsgpu_sr_gram", "pepsgpu_sr_weighted_sum", "pepsgpu_sr_copy_samples",
    "pepsgpu_opt_begin", "pepsgpu_opt_end", "pepsgpu_opt_gradient_from_accumulators", "pepsgpu_opt_set_gradient",
    "pepsgpu_opt_get_gradient", "pepsgpu_opt_clip", "pepsgpu_opt_natural_gradient", "pepsgpu_opt_step", "pepsgpu_opt_scale_state",
    "pepsgpu_opt_read_state", "pepsgpu_fermion_decoration_set", "pepsgpu_minsr_direction", "pepsgpu_diag_eigh",
    "pepsgpu_vmc_snapshot_save", "pepsgpu_vmc_snapshot_read", "pepsgpu_vmc_snapshot_clear",
    "pepsgpu_guard_base_save", "pepsgpu_guard_base_restore", "pepsgpu_guard_base_clear", "pepsgpu_guard_preview",
    "pepsgpu_lbfgs_begin", "pepsgpu_lbfgs_end", "pepsgpu_lbfgs_reset", "pepsgpu_lbfgs_update", "pepsgpu_lbfgs_direction",
    "pepsgpu_lbfgs_trial", "pepsgpu_lbfgs_slope", "pepsgpu_lbfgs_commit", "pepsgpu_lbfgs_get_direction", "pepsgpu_lbfgs_get_pair",
    "pepsgpu_lbfgs_counters",
    "pepsgpu_update_local", "pepsgpu_erase_envs_after_update", "pepsgpu_evaluate_amplitude",
    "pepsgpu_walker_flags", "pepsgpu_sync", "pepsgpu_stats", "pepsgpu_profile_enable", "pepsgpu_profile_read",
    "pepsgpu_diag_tgemm", "pepsgpu_diag_tgemm_desc", "pepsgpu_diag_tgemm_route", "pepsgpu_diag_tgemm_chain", "pepsgpu_diag_tgemm_chain3", "pepsgpu_diag_chol", "pepsgpu_diag_chol_adaptive", "pepsgpu_diag_chol_pivot", "pepsgpu_diag_rows_qr", "pepsgpu_diag_suwa_todo", "pepsgpu_diag_dot4", "pepsgpu_diag_gram_chol", "pepsgpu_diag_gram_chol_wave", "pepsgpu_diag_gram_cols", "pepsgpu_diag_gram_rows", "pepsgpu_diag_mgemm_dense", "pepsgpu_diag_jacobi", "pepsgpu_diag_trunc_rows", "pepsgpu_version",
    "pepsgpu_diag_chol_solve_rows", "pepsgpu_diag_gather_rows", "pepsgpu_diag_sign_table", "pepsgpu_diag_truncate_site",
    "pepsgpu_diag_tgemm_chain_pair", "pepsgpu_diag_chain_d8_launches", "pepsgpu_diag_chain_d8_stats",
]


def load_library(path=LIB_PATH):
    if not os.path.exists(path):
        raise ImportError("libpepsgpu.so not built (%s): run `python -c 'import __graft_entry__ as g; g.build()'`" % path)
    lib = C.CDLL(path)
    vp, ip, dp = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)
    lib.pepsgpu_ctx_create.argtypes = [C.POINTER(vp)] + [C.c_int] * 8 + [C.c_double, C.c_int, C.c_int]
    lib.pepsgpu_set_truncate_params.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_int, C.c_double, C.c_int]
    lib.pepsgpu_ctx_destroy.argtypes = [vp]
    lib.pepsgpu_ctx_destroy.restype = None
    lib.pepsgpu_last_error.argtypes = [vp]
    lib.pepsgpu_last_error.restype = C.c_char_p
    lib.pepsgpu_version.restype = C.c_char_p
    lib.pepsgpu_state_upload.argtypes = [vp, vp, C.c_int]
    lib.pepsgpu_walkers_set_configs.argtypes = [vp, C.c_int, ip]
    lib.pepsgpu_walkers_get_configs.argtypes = [vp, ip]
    lib.pepsgpu_n_walkers.argtypes = [vp]
    for name in ("grow_bmps_step", "grow_full_bmps", "grow_bmps_for_row", "grow_bmps_for_col", "shift_bmps_window",
                 "delete_inner_bmps", "generate_bmps_approach", "bmps_stack_size", "bten_stack_size",
                 "grow_bten_step", "shift_bten_window"):
        getattr(lib, "pepsgpu_" + name).argtypes = [vp, C.c_int]
    lib.pepsgpu_bmps_park.argtypes = [vp, C.c_int, C.c_int]
    lib.pepsgpu_bmps_unpark.argtypes = [vp, C.c_int]
    lib.pepsgpu_get_bmps_tensor.argtypes = [vp, C.c_int, C.c_int, C.c_int, ip, dp, dp]
    lib.pepsgpu_init_bten.argtypes = [vp, C.c_int, C.c_int]
    lib.pepsgpu_truncate_bten.argtypes = [vp, C.c_int, C.c_int]
    lib.pepsgpu_grow_full_bten.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.pepsgpu_trace.argtypes = [vp, C.c_int, C.c_int, C.c_int, dp]
    lib.pepsgpu_replace_nn_trace.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, ip, dp]
    lib.pepsgpu_replace_one_trace.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, ip, dp]
    lib.pepsgpu_punch_hole.argtypes = [vp, C.c_int, C.c_int, C.c_int, dp]
    lib.pepsgpu_trace_scaling.argtypes = [vp, C.c_int]
    for name in ("init_bten2", "grow_bten2_step", "shift_bten2_window"):
        getattr(lib, "pepsgpu_" + name).argtypes = [vp, C.c_int, C.c_int]
    lib.pepsgpu_grow_full_bten2.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.pepsgpu_bten2_stack_size.argtypes = [vp, C.c_int]
    lib.pepsgpu_replace_nnn_trace.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, ip, dp]
    lib.pepsgpu_bten2_select_set.argtypes = [vp, C.c_int]
    lib.pepsgpu_cfg_override_slice.argtypes = [vp, C.c_int, C.c_int, ip]
    lib.pepsgpu_replace_plaquette_trace.argtypes = [vp, C.c_int, C.c_int, C.c_int, ip, C.c_int, C.c_int, dp]
    lib.pepsgpu_replace_tnn_trace.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, ip, dp]
    lib.pepsgpu_replace_sqrt5_trace.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, ip, dp]
    lib.pepsgpu_grad_reset.argtypes = [vp]
    lib.pepsgpu_grad_accumulate.argtypes = [vp, dp, dp, C.c_int]
    lib.pepsgpu_grad_accumulate_states.argtypes = [vp, dp, dp, C.c_int, ip]
    lib.pepsgpu_grad_read.argtypes = [vp, dp, dp]
    lib.pepsgpu_grad_device_ptr.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_long)]
    lib.pepsgpu_grad_allreduce.argtypes = [vp]
    lib.pepsgpu_bcast_state.argtypes = [vp, C.c_int]
    lib.pepsgpu_comm_unique_id.argtypes = [vp]
    lib.pepsgpu_comm_init.argtypes = [vp, C.c_int, C.c_int, vp]
    lib.pepsgpu_comm_size.argtypes = [vp]
    lib.pepsgpu_comm_rank.argtypes = [vp]
    lib.pepsgpu_comm_destroy.argtypes = [vp]
    lib.pepsgpu_allreduce.argtypes = [vp, vp, C.c_long, C.c_int, C.c_int, C.c_int]
    lib.pepsgpu_sweep_slice_exchange.argtypes = [vp, C.c_int, C.c_int, C.c_int, dp, dp, ip, ip, ip]
    lib.pepsgpu_sweep_slice_exchange_tab.argtypes = [vp, C.c_int, C.c_int, C.c_int, dp, ip, dp, ip, ip, ip]
    lib.pepsgpu_sweep_slice_fullspace.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32), dp, ip, ip]
    lib.pepsgpu_sweep_slice_tnn3.argtypes = [vp, C.c_int, C.c_int, ip, C.c_int, C.POINTER(C.c_uint32), dp, ip, ip, ip]
    lib.pepsgpu_diag_tnn3_table.argtypes = [C.c_int, ip]
    lib.pepsgpu_nn_exchange_slice.argtypes = [vp, C.c_int, C.c_int, C.c_int, dp, dp]
    lib.pepsgpu_nn_exchange_slice_tab.argtypes = [vp, C.c_int, C.c_int, C.c_int, ip, C.c_int, dp, dp]
    lib.pepsgpu_nnn_exchange_slice.argtypes = [vp, C.c_int, C.c_int, dp]
    lib.pepsgpu_diag_nnn_slice_calls.argtypes = []
    lib.pepsgpu_diag_nnn_slice_calls.restype = C.c_long
    lib.pepsgpu_nnn_hop_slice_fermion.argtypes = [vp, C.c_int, C.c_int, ip, C.c_int, dp, dp]
    lib.pepsgpu_diag_nnn_hop_slice_calls.argtypes = []
    lib.pepsgpu_diag_nnn_hop_slice_calls.restype = C.c_long
    lib.pepsgpu_diag_fermion_hop_cand.argtypes = [C.c_int, C.c_int, C.c_int, ip, C.c_int, ip, C.c_int, C.c_int, ip, ip, ip]
    lib.pepsgpu_nn_pair_slice_fermion.argtypes = [vp, C.c_int, C.c_int, C.c_int, ip, ip, ip, dp, dp, dp]
    lib.pepsgpu_diag_pair_slice_calls.argtypes = []
    lib.pepsgpu_diag_pair_slice_calls.restype = C.c_long
    lib.pepsgpu_diag_pair_cand.argtypes = [C.c_int, C.c_int, C.c_int, ip, ip, C.c_int, ip, C.c_int, C.c_int, C.c_int, ip, ip]
    lib.pepsgpu_nn_hop_slice_fermion.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, ip, ip, dp, dp]
    lib.pepsgpu_diag_hop_slice_calls.argtypes = []
    lib.pepsgpu_diag_hop_slice_calls.restype = C.c_long
    lib.pepsgpu_sweep_slice_sector.argtypes = [vp, C.c_int, C.c_int, C.c_int, ip, C.c_int, ip, C.c_int, C.POINTER(C.c_uint32), dp, ip, ip, ip]
    lib.pepsgpu_diag_sector_slice_calls.argtypes = []
    lib.pepsgpu_diag_sector_slice_calls.restype = C.c_long
    lib.pepsgpu_diag_sector_cand.argtypes = [C.c_int, C.c_int, C.c_int, ip, C.c_int, ip, C.c_int, ip, C.c_int, C.c_int, C.c_int, ip, ip]
    lib.pepsgpu_link_exchange_slice.argtypes = [vp, C.c_int, C.c_int, C.c_int, dp]
    lib.pepsgpu_diag_link_slice_calls.argtypes = []
    lib.pepsgpu_diag_link_slice_calls.restype = C.c_long
    lib.pepsgpu_diag_link_cand.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, ip, C.c_int, C.c_int, C.c_int, ip, ip]
    lib.pepsgpu_diag_dot4.argtypes = [C.c_int, vp, vp, ip, C.c_int, dp, ip, dp]
    lib.pepsgpu_onsite_slice.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, ip, dp, dp]
    lib.pepsgpu_walker_create.argtypes = [vp, C.c_int, C.c_int, ip]
    lib.pepsgpu_walker_clone.argtypes = [vp, C.c_int, ip]
    lib.pepsgpu_walker_destroy.argtypes = [vp, C.c_int]
    lib.pepsgpu_walker_info.argtypes = [vp, C.c_int, ip, ip, ip, ip]
    lib.pepsgpu_walker_set_mpo.argtypes = [vp, C.c_int, C.c_int, ip, dp, C.c_int]
    u8p = C.POINTER(C.c_uint8)
    lib.pepsgpu_walker_set_mpo_excited.argtypes = [vp, C.c_int, C.c_int, C.c_int, ip, u8p]
    lib.pepsgpu_walker_trace_slice.argtypes = [vp, C.c_int, C.c_int, ip, u8p, dp]
    lib.pepsgpu_diag_walker_slice_calls.argtypes = []
    lib.pepsgpu_diag_walker_slice_calls.restype = C.c_long
    lib.pepsgpu_walker_set_mpo_excited_pair.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, ip, ip, C.c_int, u8p, ip]
    lib.pepsgpu_walker_pair_trace_slice.argtypes = [vp, C.c_int, C.c_int, C.c_int, ip, ip, u8p, dp]
    lib.pepsgpu_diag_walker_pair_slice_calls.argtypes = []
    lib.pepsgpu_diag_walker_pair_slice_calls.restype = C.c_long
    lib.pepsgpu_diag_walker_pair_cand.argtypes = [C.c_int, C.c_int, ip, ip, C.c_int, ip, C.c_int, C.c_int, u8p, ip, ip, ip, ip]
    lib.pepsgpu_walker_evolve.argtypes = [vp, C.c_int]
    lib.pepsgpu_walker_evolve_step.argtypes = [vp, C.c_int]
    lib.pepsgpu_walker_contract_row.argtypes = [vp, C.c_int, C.c_int, dp]
    lib.pepsgpu_walker_init_bten.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.pepsgpu_walker_grow_bten_step.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    lib.pepsgpu_walker_shift_bten_window.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    lib.pepsgpu_walker_trace_with_bten.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, ip, dp, C.c_int, dp]
    lib.pepsgpu_walker_clear_bten.argtypes = [vp, C.c_int]
    lib.pepsgpu_walker_get_bmps_tensor.argtypes = [vp, C.c_int, C.c_int, ip, dp, dp]
    lib.pepsgpu_sr_begin.argtypes = [vp, C.c_int]
    lib.pepsgpu_sr_append.argtypes = [vp, dp]
    lib.pepsgpu_sr_count.argtypes = [vp]
    lib.pepsgpu_sr_sum.argtypes = [vp, dp]
    lib.pepsgpu_sr_matvec.argtypes = [vp, dp, C.c_double, C.c_double, dp]
    lib.pepsgpu_sr_matvec_c128.argtypes = [vp, dp, C.c_double, C.c_double, C.c_double, dp]
    lib.pepsgpu_sr_cg_solve.argtypes = [vp, dp, dp, C.c_double, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double, dp, dp, ip, ip]
    lib.pepsgpu_sr_gram.argtypes = [vp, vp, vp, C.c_int, dp]
    lib.pepsgpu_sr_weighted_sum.argtypes = [vp, dp, dp]
    lib.pepsgpu_sr_copy_samples.argtypes = [vp, vp, vp]
    if hasattr(lib, "pepsgpu_opt_begin"):           # (PEPSGPU_LIB may name a build from before these entries: A/B against the parent commit)
        lib.pepsgpu_opt_begin.argtypes = [vp]
        lib.pepsgpu_opt_end.argtypes = [vp]
        lib.pepsgpu_opt_gradient_from_accumulators.argtypes = [vp, dp, C.c_double, dp, dp]
        lib.pepsgpu_opt_set_gradient.argtypes = [vp, dp]
        lib.pepsgpu_opt_get_gradient.argtypes = [vp, dp]
        lib.pepsgpu_opt_clip.argtypes = [vp, C.c_double, C.c_double, dp]
        lib.pepsgpu_opt_natural_gradient.argtypes = [vp, C.c_double, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double, dp, ip, ip, dp]
        lib.pepsgpu_opt_step.argtypes = [vp, C.c_int, C.c_double, dp, C.c_int]
        lib.pepsgpu_opt_scale_state.argtypes = [vp, C.c_double]
        lib.pepsgpu_opt_read_state.argtypes = [vp, dp]
        lib.pepsgpu_vmc_snapshot_save.argtypes = [vp]
        lib.pepsgpu_vmc_snapshot_read.argtypes = [vp, dp]
        lib.pepsgpu_vmc_snapshot_clear.argtypes = [vp]
    if hasattr(lib, "pepsgpu_guard_base_save"):     # (PEPSGPU_LIB may name a build from before these entries)
        lib.pepsgpu_guard_base_save.argtypes = [vp]
        lib.pepsgpu_guard_base_restore.argtypes = [vp]
        lib.pepsgpu_guard_base_clear.argtypes = [vp]
        lib.pepsgpu_guard_preview.argtypes = [vp, C.c_int, C.c_double, dp, C.c_int]
    if hasattr(lib, "pepsgpu_fermion_decoration_set"):
        lib.pepsgpu_fermion_decoration_set.argtypes = [vp, C.c_int, ip, C.POINTER(C.c_uint8)]
    if hasattr(lib, "pepsgpu_minsr_direction"):     # (PEPSGPU_LIB may name a build from before these entries)
        lib.pepsgpu_minsr_direction.argtypes = [vp, dp, dp, C.c_double, C.c_double, C.c_int, dp, dp]
        lib.pepsgpu_diag_eigh.argtypes = [vp, C.c_int, C.c_int, dp, dp, dp, ip]
    if hasattr(lib, "pepsgpu_lbfgs_begin"):         # (PEPSGPU_LIB may name a build from before these entries)
        lib.pepsgpu_lbfgs_begin.argtypes = [vp, C.c_int]
        lib.pepsgpu_lbfgs_end.argtypes = [vp]
        lib.pepsgpu_lbfgs_reset.argtypes = [vp]
        lib.pepsgpu_lbfgs_update.argtypes = [vp, C.c_double, C.c_int, ip, dp]
        lib.pepsgpu_lbfgs_direction.argtypes = [vp, C.c_double, C.c_double, dp, dp, ip]
        lib.pepsgpu_lbfgs_trial.argtypes = [vp, C.c_double]
        lib.pepsgpu_lbfgs_slope.argtypes = [vp, dp]
        lib.pepsgpu_lbfgs_commit.argtypes = [vp]
        lib.pepsgpu_lbfgs_get_direction.argtypes = [vp, dp]
        lib.pepsgpu_lbfgs_get_pair.argtypes = [vp, C.c_int, dp, dp]
        lib.pepsgpu_lbfgs_counters.argtypes = [vp, C.POINTER(C.c_long)]
    lib.pepsgpu_update_local.argtypes = [vp, C.c_int, ip, ip, C.POINTER(C.c_uint8)]
    lib.pepsgpu_erase_envs_after_update.argtypes = [vp, C.c_int, C.c_int]
    lib.pepsgpu_evaluate_amplitude.argtypes = [vp, dp]
    lib.pepsgpu_walker_flags.argtypes = [vp, ip]
    lib.pepsgpu_sync.argtypes = [vp]
    lib.pepsgpu_stats.argtypes = [vp, dp, C.c_int]
    lib.pepsgpu_profile_enable.argtypes = [vp, C.c_int]
    lib.pepsgpu_profile_read.argtypes = [vp, dp]
    lib.pepsgpu_diag_tgemm.argtypes = [C.c_int, C.c_int, ip, C.c_int, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t,
                                       C.c_int, C.c_long, C.c_long, C.c_long]
    lp, ullp = C.POINTER(C.c_long), C.POINTER(C.c_ulonglong)
    lib.pepsgpu_diag_tgemm_desc.argtypes = [C.c_int, ip, C.c_int, lp, C.c_int, dp, C.c_int, ip, C.c_long, C.POINTER(C.c_float),
                                            vp, C.c_size_t, C.c_long, vp, C.c_size_t, C.c_long, vp, C.c_size_t,
                                            C.POINTER(C.c_float), dp, ip, ip, ullp]
    lib.pepsgpu_diag_tgemm_route.argtypes = [C.c_int, ip, C.c_int, lp, C.c_int, dp, C.c_int, C.c_long, C.c_long, ip]
    lib.pepsgpu_diag_tgemm_chain3.argtypes = [ip, ip, C.c_long, C.c_int, ip, C.c_int, ip, ip, C.c_int, ip, vp, vp, vp, vp, vp,
                                              ip, ip, ip]
    lib.pepsgpu_diag_chol.argtypes = [C.c_int, dp, C.c_int, C.c_int, vp]
    lib.pepsgpu_diag_chol_adaptive.argtypes = [C.c_int, dp, C.c_int, C.c_int, vp, ip]
    lib.pepsgpu_diag_gram_chol.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, ip]
    lib.pepsgpu_diag_jacobi.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, ip]
    if hasattr(lib, "pepsgpu_diag_trunc_rows"):     # (PEPSGPU_LIB may name a build from before the entry: A/B against the parent commit)
        lib.pepsgpu_diag_trunc_rows.argtypes = [vp, C.c_int, C.c_int, C.c_int, ip, C.c_int, C.c_int, vp, ip, ip]
    if hasattr(lib, "pepsgpu_diag_truncate_site"):  # (PEPSGPU_LIB may name a build from before these entries)
        lib.pepsgpu_diag_chol_solve_rows.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, ip, C.c_int, ip]
        lib.pepsgpu_diag_gather_rows.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.c_int, ip, C.c_int, ip, ip, vp]
        lib.pepsgpu_diag_sign_table.argtypes = [C.c_int, C.c_int, C.c_int, vp]
        lib.pepsgpu_diag_truncate_site.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, ip, C.c_int, vp, ip, ip]
    return lib


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = load_library()
    return _lib


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class _ReapingLib:
    """The library as a Context sees it: looking a function up first frees the BMPSWalker ids whose Python objects were finalised
    since the last call (Walker.__del__ only queues them), so the release happens on the thread that uses the context, between two
    calls, and before the next one can observe the walker."""

    def __init__(self, raw, ctx):
        object.__setattr__(self, "_raw", raw)
        object.__setattr__(self, "_ctx", ctx)

    def __getattr__(self, name):
        ctx = object.__getattribute__(self, "_ctx")
        raw = object.__getattribute__(self, "_raw")
        dead = ctx.__dict__.get("_dead_walkers")
        if dead and name != "pepsgpu_ctx_destroy":
            h = ctx.__dict__.get("_h")
            while dead and h:
                raw.pepsgpu_walker_destroy(h, dead.pop())
        return getattr(raw, name)


class Context:
    """Thin RAII wrapper of a pepsgpu_ctx: one walker batch on one GPU."""

    def __init__(self, rows, cols, D, phys_dim, chi, dtype=F32, device=0, max_walkers=256, chi_min=None,
                 trunc_err=0.0, scheme=0, convergence_tol=None, iter_max=None):
        self._l = _ReapingLib(lib(), self)
        self._dead_walkers = []
        self.rows, self.cols, self.D, self.d = rows, cols, D, phys_dim
        self.dtype = dtype
        self.chi = chi
        self._ot = np.complex128 if dtype == C128 else np.float64      # type of every scalar / tensor the calls return
        h = C.c_void_p()
        rc = self._l.pepsgpu_ctx_create(C.byref(h), device, dtype, rows, cols, D, phys_dim,
                                        chi if chi_min is None else chi_min, chi, trunc_err, scheme, max_walkers)
        if rc != 0:
            raise _ERR.get(rc, RuntimeError)("pepsgpu_ctx_create failed (%d): %s"
                                             % (rc, self._l.pepsgpu_last_error(None).decode()))
        self._h = h
        self.n = 0
        if scheme != SVD_COMPRESS and convergence_tol is not None:
            self.set_truncate_params(chi if chi_min is None else chi_min, chi, trunc_err, scheme, convergence_tol, iter_max)

    def close(self):
        if getattr(self, "_h", None):
            self._l.pepsgpu_ctx_destroy(self._h)      # (drops every BMPSWalker of the context with it)
            self._h = None
        self._dead_walkers = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            raise _ERR.get(rc, RuntimeError)("pepsgpu error %d: %s" % (rc, self._l.pepsgpu_last_error(self._h).decode()))

    # -- state / walkers --
    def set_truncate_params(self, chi_min, chi_max, trunc_err=0.0, scheme=0, convergence_tol=0.0, iter_max=0):
        """BMPSContractor::SetTruncateParams (bmps_contractor.h:216); scheme 0 SVD, 1 Variational2Site, 2 Variational1Site."""
        self._ck(self._l.pepsgpu_set_truncate_params(self._h, chi_min, chi_max, trunc_err, scheme, convergence_tol, iter_max))
        self.chi = chi_max

    def state_upload(self, flat):
        flat = np.ascontiguousarray(flat)
        assert flat.shape == (self.rows, self.cols, self.d, self.D, self.D, self.D, self.D), flat.shape
        if np.iscomplexobj(flat):
            if self.dtype != C128:
                raise ValueError("a complex state needs a complex context (dtype=C128)")
            hd, flat = C128, np.ascontiguousarray(flat, dtype=np.complex128)
        else:
            hd = F32 if flat.dtype == np.float32 else F64
            if hd == F64:
                flat = flat.astype(np.float64, copy=False)
        self._ck(self._l.pepsgpu_state_upload(self._h, flat.ctypes.data_as(C.c_void_p), hd))

    def set_configs(self, configs):
        cfg = np.ascontiguousarray(configs, dtype=np.int32)
        assert cfg.ndim == 3 and cfg.shape[1:] == (self.rows, self.cols)
        self._ck(self._l.pepsgpu_walkers_set_configs(self._h, cfg.shape[0], _ip(cfg)))
        self.n = cfg.shape[0]

    def get_configs(self):
        out = np.zeros((self.n, self.rows, self.cols), dtype=np.int32)
        self._ck(self._l.pepsgpu_walkers_get_configs(self._h, _ip(out)))
        return out

    # -- contractor mirror --
    def grow_bmps_step(self, pos): self._ck(self._l.pepsgpu_grow_bmps_step(self._h, pos))
    def grow_full_bmps(self, pos): self._ck(self._l.pepsgpu_grow_full_bmps(self._h, pos))
    def grow_bmps_for_row(self, row): self._ck(self._l.pepsgpu_grow_bmps_for_row(self._h, row))
    def grow_bmps_for_col(self, col): self._ck(self._l.pepsgpu_grow_bmps_for_col(self._h, col))
    def shift_bmps_window(self, pos): self._ck(self._l.pepsgpu_shift_bmps_window(self._h, pos))
    def delete_inner_bmps(self, pos): self._ck(self._l.pepsgpu_delete_inner_bmps(self._h, pos))
    def bmps_park(self, pos, keep): self._ck(self._l.pepsgpu_bmps_park(self._h, pos, keep))
    def bmps_unpark(self, pos): self._ck(self._l.pepsgpu_bmps_unpark(self._h, pos))
    def generate_bmps_approach(self, pos): self._ck(self._l.pepsgpu_generate_bmps_approach(self._h, pos))
    def bmps_stack_size(self, pos): return self._l.pepsgpu_bmps_stack_size(self._h, pos)
    def bten_stack_size(self, pos): return self._l.pepsgpu_bten_stack_size(self._h, pos)
    def init_bten(self, pos, slice_num): self._ck(self._l.pepsgpu_init_bten(self._h, pos, slice_num))
    def grow_full_bten(self, pos, slice_num, remain_sites=2, init=True):
        self._ck(self._l.pepsgpu_grow_full_bten(self._h, pos, slice_num, remain_sites, int(init)))
    def grow_bten_step(self, pos): self._ck(self._l.pepsgpu_grow_bten_step(self._h, pos))
    def shift_bten_window(self, pos): self._ck(self._l.pepsgpu_shift_bten_window(self._h, pos))
    def truncate_bten(self, pos, length): self._ck(self._l.pepsgpu_truncate_bten(self._h, pos, length))

    def get_bmps_tensor(self, pos, level, idx):
        dims = np.zeros(3, dtype=np.int32)
        self._ck(self._l.pepsgpu_get_bmps_tensor(self._h, pos, level, idx, _ip(dims), None, None))
        data = np.zeros((self.n,) + tuple(int(x) for x in dims), dtype=self._ot)
        ls = np.zeros(self.n, dtype=np.float64)
        self._ck(self._l.pepsgpu_get_bmps_tensor(self._h, pos, level, idx, _ip(dims), _dp(data), _dp(ls)))
        return data, ls

    def sweep_slice_exchange(self, orientation, slice_num, uniforms, amplitude, pair_table=None):
        """one row / column of the NN-exchange sweep on the device; uniforms [n][nu] (next deviates of each walker's stream);
        pair_table [d * d][2] (optional): the pair of states the move proposes for the states (a, b) of a bond (fermionic extended
        states); returns (amplitude, consumed [n], accepted [n], slice_states [n][N])"""
        u = np.ascontiguousarray(uniforms, dtype=np.float64)
        assert u.ndim == 2 and u.shape[0] == self.n
        amp = np.array(amplitude, dtype=self._ot)
        N = self.cols if orientation == HORIZONTAL else self.rows
        cons, acc = np.zeros(self.n, dtype=np.int32), np.zeros(self.n, dtype=np.int32)
        st = np.zeros((self.n, N), dtype=np.int32)
        if pair_table is None:
            self._ck(self._l.pepsgpu_sweep_slice_exchange(self._h, orientation, slice_num, u.shape[1], _dp(u), _dp(amp), _ip(cons), _ip(acc), _ip(st)))
        else:
            tab = np.ascontiguousarray(pair_table, dtype=np.int32)
            assert tab.shape == (self.d * self.d, 2), tab.shape
            self._ck(self._l.pepsgpu_sweep_slice_exchange_tab(self._h, orientation, slice_num, u.shape[1], _dp(u), _ip(tab), _dp(amp), _ip(cons),
                                                              _ip(acc), _ip(st)))
        return amp, cons, acc, st

    def sweep_slice_fullspace(self, orientation, slice_num, phys_dim, engine_words, amplitude):
        """one row / column of the full-space NN updater (Suwa-Todo over phys_dim^2 states per bond) on the device; engine_words
        [n][2 (N - 1)] uint32 = the next raw outputs of each walker's mt19937; returns (amplitude, accepted [n], slice_states [n][N])"""
        N = self.cols if orientation == HORIZONTAL else self.rows
        wd = np.ascontiguousarray(engine_words, dtype=np.uint32)
        assert wd.shape == (self.n, 2 * (N - 1)), wd.shape
        amp = np.array(amplitude, dtype=self._ot)
        acc = np.zeros(self.n, dtype=np.int32)
        st = np.zeros((self.n, N), dtype=np.int32)
        self._ck(self._l.pepsgpu_sweep_slice_fullspace(self._h, orientation, slice_num, phys_dim, wd.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                       _dp(amp), _ip(acc), _ip(st)))
        return amp, acc, st

    def sweep_slice_tnn3(self, orientation, slice_num, engine_words, triple_table=None):
        """one row / column of the three-site exchange updater on the device; engine_words [n][n_words] uint32 (n_words >= 2 (N - 2)) =
        the next raw outputs of each walker's mt19937; triple_table [d^3][20] (None: the bosonic table of the context's d); returns
        (amplitude [n] after the slice, consumed words [n], accepted moves [n], slice_states [n][N])"""
        N = self.cols if orientation == HORIZONTAL else self.rows
        wd = np.ascontiguousarray(engine_words, dtype=np.uint32)
        assert wd.ndim == 2 and wd.shape[0] == self.n, wd.shape
        amp = np.zeros(self.n, dtype=self._ot)
        cons, acc = np.zeros(self.n, dtype=np.int32), np.zeros(self.n, dtype=np.int32)
        st = np.zeros((self.n, N), dtype=np.int32)
        tab = None
        if triple_table is not None:
            tab = np.ascontiguousarray(triple_table, dtype=np.int32)
            assert tab.shape == (self.d ** 3, 20), tab.shape
        self._ck(self._l.pepsgpu_sweep_slice_tnn3(self._h, orientation, slice_num, None if tab is None else _ip(tab), wd.shape[1],
                                                  wd.ctypes.data_as(C.POINTER(C.c_uint32)), _dp(amp), _ip(cons), _ip(acc), _ip(st)))
        return amp, cons, acc, st

    def nn_exchange_slice(self, orientation, slice_num, punch_holes=False):
        """psi [n] and the amplitudes with the two sites of every bond of the slice exchanged [n][N-1], one read-back"""
        N = self.cols if orientation == HORIZONTAL else self.rows
        psi, ex = np.zeros(self.n), np.zeros((self.n, N - 1))
        self._ck(self._l.pepsgpu_nn_exchange_slice(self._h, orientation, slice_num, int(punch_holes), _dp(psi), _dp(ex)))
        return psi, ex

    def nn_exchange_slice_tab(self, orientation, slice_num, punch_holes=False, pair_table=None, psi_per_bond=False):
        """the exchange slice of every element type: pair_table [d * d][2] (None: the swap); returns (psi, psi_ex [n][N-1]) with
        psi [n], or [n][N-1] (the Trace before every bond's replacement trace) when psi_per_bond"""
        N = self.cols if orientation == HORIZONTAL else self.rows
        psi = np.zeros((self.n, N - 1) if psi_per_bond else self.n, dtype=self._ot)
        ex = np.zeros((self.n, N - 1), dtype=self._ot)
        tab = None
        if pair_table is not None:
            tab = np.ascontiguousarray(pair_table, dtype=np.int32)
            assert tab.shape == (self.d * self.d, 2), tab.shape
        self._ck(self._l.pepsgpu_nn_exchange_slice_tab(self._h, orientation, slice_num, int(punch_holes), _ip(tab) if tab is not None else None,
                                                       int(psi_per_bond), _dp(psi), _dp(ex)))
        return psi, ex

    def nnn_exchange_slice(self, row1, diag_mask=3):
        """the diagonal bonds of the row pair (row1, row1 + 1): [n][cols - 1][2] amplitudes with the two ends of the diagonal exchanged
        (kind 0 LEFTUP_TO_RIGHTDOWN, kind 1 LEFTDOWN_TO_RIGHTUP; diag_mask bit per kind), 0 for a masked-off diagonal and for equal
        end states; one read-back"""
        val = np.zeros((self.n, self.cols - 1, 2), dtype=self._ot)
        self._ck(self._l.pepsgpu_nnn_exchange_slice(self._h, row1, diag_mask, _dp(val)))
        return val

    def link_exchange_slice(self, orient, slice1, link_mask):
        """the links of the row pair (HORIZONTAL, slice1 = row r) or column pair (VERTICAL, slice1 = column c): [n][N - 1][4] amplitudes
        with the two end states of link `kind` of the window at position j exchanged (N = cols / rows).  HORIZONTAL kinds: 0 diagonal
        (r, c)-(r+1, c+1), 1 diagonal (r+1, c)-(r, c+1), 2 flat link (r, c)-(r+1, c+2), 3 flat link (r+1, c)-(r, c+2); VERTICAL kinds: 2
        steep link (r, c)-(r+2, c+1), 3 steep link (r+2, c)-(r, c+1).  link_mask has one bit per kind; 0 for a masked-off kind, equal end
        states and a position without such a link; one read-back"""
        N = self.cols if orient == HORIZONTAL else self.rows
        val = np.zeros((self.n, max(N - 1, 1), 4), dtype=self._ot)
        self._ck(self._l.pepsgpu_link_exchange_slice(self._h, orient, slice1, link_mask, _dp(val)))
        return val

    def nnn_hop_slice_fermion(self, row1, nf, diag_mask=3):
        """the diagonal hops of the row pair (row1, row1 + 1) of a fermionic state (extended row-major configurations; nf [d] the
        fermion number of each physical state, 4 d = the context's physical dimension): (psi [n][cols - 1], val [n][cols - 1][2]) with
        val = jw psi' of each diagonal (kind 0 LEFTUP_TO_RIGHTDOWN, kind 1 LEFTDOWN_TO_RIGHTUP), 0 for a masked-off diagonal and a
        forbidden hop (equal occupation at the two ends); psi is 0 for a plaquette without any allowed hop; one read-back"""
        occ = np.ascontiguousarray(nf, dtype=np.int32)
        psi = np.zeros((self.n, self.cols - 1), dtype=self._ot)
        val = np.zeros((self.n, self.cols - 1, 2), dtype=self._ot)
        self._ck(self._l.pepsgpu_nnn_hop_slice_fermion(self._h, row1, occ.size, _ip(occ), diag_mask, _dp(psi), _dp(val)))
        return psi, val

    def nn_pair_slice_fermion(self, orientation, slice_num, nf, pair_table, exchange_table=None):
        """one row / column of a fermionic state (extended configurations of the pass's mode order; nf [d] the fermion number of each
        physical state, 4 d = the context's physical dimension): pair_table [d * d][2][2] over physical states, candidate k of the pair
        (a, b) or (-1, -1); exchange_table [(4 d)^2][2] over extended states or None.  Returns (psi [n][N-1], ex [n][N-1] or None,
        pair [n][N-1][2]) with pair = sign psi' (sign -1 where the fermion number changes by +-2), exactly 0 for "no candidate"; one
        read-back"""
        occ = np.ascontiguousarray(nf, dtype=np.int32)
        tab = np.ascontiguousarray(pair_table, dtype=np.int32)
        assert tab.size == occ.size * occ.size * 4, tab.shape
        N = self.cols if orientation == HORIZONTAL else self.rows
        psi = np.zeros((self.n, N - 1), dtype=self._ot)
        pair = np.zeros((self.n, N - 1, 2), dtype=self._ot)
        xt, ex = None, None
        if exchange_table is not None:
            xt = np.ascontiguousarray(exchange_table, dtype=np.int32)
            assert xt.shape == (self.d * self.d, 2), xt.shape
            ex = np.zeros((self.n, N - 1), dtype=self._ot)
        self._ck(self._l.pepsgpu_nn_pair_slice_fermion(self._h, orientation, slice_num, occ.size, _ip(occ), _ip(tab),
                                                       _ip(xt) if xt is not None else None, _dp(psi),
                                                       _dp(ex) if ex is not None else None, _dp(pair)))
        return psi, ex, pair

    def nn_hop_slice_fermion(self, orientation, slice_num, nf, hop_table, punch_holes=False):
        """one row / column of a fermionic state with up to two hop candidates per bond (the Hubbard model): hop_table [d * d][2][2] over
        physical states as the pair_table of nn_pair_slice_fermion.  punch_holes: the row pass of the energy evaluation, the hole of
        every site of the slice goes into HBM and the window is shifted after the last bond too.  Returns (psi [n][N-1], hop [n][N-1][2]),
        hop exactly 0 for "no candidate"; one read-back"""
        occ = np.ascontiguousarray(nf, dtype=np.int32)
        tab = np.ascontiguousarray(hop_table, dtype=np.int32)
        assert tab.size == occ.size * occ.size * 4, tab.shape
        N = self.cols if orientation == HORIZONTAL else self.rows
        psi = np.zeros((self.n, N - 1), dtype=self._ot)
        hop = np.zeros((self.n, N - 1, 2), dtype=self._ot)
        self._ck(self._l.pepsgpu_nn_hop_slice_fermion(self._h, orientation, slice_num, int(punch_holes), occ.size, _ip(occ), _ip(tab),
                                                      _dp(psi), _dp(hop)))
        return psi, hop

    def sweep_slice_sector(self, orientation, slice_num, sector_table, engine_words, amplitude, nf=None):
        """one row / column of Suwa-Todo moves inside the tabulated sector of each bond (MCUpdateSquareNNHubbardU1U1OBC) on the device:
        sector_table [d * d][2 + 2 max_cand] over physical states (m, init, max_cand slots, unused ones (-1, -1)); nf [d] the fermion
        number of each physical state for a fermionic context (4 d = its physical dimension), None for a bosonic one (d = its physical
        dimension); engine_words [n][n_words] uint32 (n_words >= 2 (N - 1)) = the next raw outputs of each walker's mt19937.  Returns
        (amplitude [n] after the slice, consumed words [n], accepted moves [n], slice_states [n][N])"""
        N = self.cols if orientation == HORIZONTAL else self.rows
        tab = np.ascontiguousarray(sector_table, dtype=np.int32)
        occ = None if nf is None else np.ascontiguousarray(nf, dtype=np.int32)
        d = self.d if occ is None else occ.size
        assert tab.ndim == 2 and tab.shape[0] == d * d and tab.shape[1] >= 4 and tab.shape[1] % 2 == 0, tab.shape
        wd = np.ascontiguousarray(engine_words, dtype=np.uint32)
        assert wd.ndim == 2 and wd.shape[0] == self.n, wd.shape
        amp = np.array(amplitude, dtype=self._ot)
        assert amp.shape == (self.n,), amp.shape
        cons, acc = np.zeros(self.n, dtype=np.int32), np.zeros(self.n, dtype=np.int32)
        st = np.zeros((self.n, N), dtype=np.int32)
        self._ck(self._l.pepsgpu_sweep_slice_sector(self._h, orientation, slice_num, d, None if occ is None else _ip(occ),
                                                    (tab.shape[1] - 2) // 2, _ip(tab), wd.shape[1],
                                                    wd.ctypes.data_as(C.POINTER(C.c_uint32)), _dp(amp), _ip(cons), _ip(acc), _ip(st)))
        return amp, cons, acc, st

    def onsite_slice(self, orientation, slice_num, site_table, punch_holes=False):
        """one-site moves along a row / column: site_table [d][n_cand] (candidate k of state s); returns (psi [n],
        psi_cand [n][N][n_cand])"""
        tab = np.ascontiguousarray(site_table, dtype=np.int32)
        assert tab.ndim == 2 and tab.shape[0] == self.d, tab.shape
        N = self.cols if orientation == HORIZONTAL else self.rows
        psi = np.zeros(self.n, dtype=self._ot)
        cand = np.zeros((self.n, N, tab.shape[1]), dtype=self._ot)
        self._ck(self._l.pepsgpu_onsite_slice(self._h, orientation, slice_num, int(punch_holes), tab.shape[1], _ip(tab), _dp(psi), _dp(cand)))
        return psi, cand

    def get_walker(self, pos, level=-1):
        """BMPSContractor::GetWalker(tn, pos) (bmps_walker.h:51-58): a Walker object forked from the top of stack `pos`
        (level >= 0: from that level of the stack, BMPSWalker(tn, stack[level], pos, level + 1, params))"""
        wid = np.zeros(1, dtype=np.int32)
        self._ck(self._l.pepsgpu_walker_create(self._h, pos, level, _ip(wid)))
        return Walker(self, int(wid[0]))

    def trace(self, row, col, bond_dir):
        out = np.zeros(self.n, dtype=self._ot)
        self._ck(self._l.pepsgpu_trace(self._h, row, col, bond_dir, _dp(out)))
        return out

    def replace_nn_trace(self, row, col, bond_dir, cand_states):
        cand = np.ascontiguousarray(cand_states, dtype=np.int32)
        assert cand.ndim == 3 and cand.shape[0] == self.n and cand.shape[2] == 2
        out = np.zeros((self.n, cand.shape[1]), dtype=self._ot)
        self._ck(self._l.pepsgpu_replace_nn_trace(self._h, row, col, bond_dir, cand.shape[1], _ip(cand), _dp(out)))
        return out

    def replace_one_trace(self, row, col, orient, cand_states):
        cand = np.ascontiguousarray(cand_states, dtype=np.int32)
        assert cand.ndim == 2 and cand.shape[0] == self.n
        out = np.zeros((self.n, cand.shape[1]), dtype=self._ot)
        self._ck(self._l.pepsgpu_replace_one_trace(self._h, row, col, orient, cand.shape[1], _ip(cand), _dp(out)))
        return out

    # -- two-row environments, NNN / third-neighbour / sqrt(5) traces --
    def init_bten2(self, pos, slice_num1): self._ck(self._l.pepsgpu_init_bten2(self._h, pos, slice_num1))
    def grow_full_bten2(self, pos, slice_num1, remain_sites=2, init=True):
        self._ck(self._l.pepsgpu_grow_full_bten2(self._h, pos, slice_num1, remain_sites, int(init)))
    def grow_bten2_step(self, pos, slice_num1): self._ck(self._l.pepsgpu_grow_bten2_step(self._h, pos, slice_num1))
    def shift_bten2_window(self, pos, slice_num1): self._ck(self._l.pepsgpu_shift_bten2_window(self._h, pos, slice_num1))
    def bten2_stack_size(self, pos): return self._l.pepsgpu_bten2_stack_size(self._h, pos)

    def _cand(self, cand_states, ncols):
        """cand_states None -> no replacement (out [n]); else [n][n_cand][ncols] -> out [n][n_cand]"""
        if cand_states is None:
            return 0, None, np.zeros(self.n, dtype=self._ot)
        cand = np.ascontiguousarray(cand_states, dtype=np.int32)
        assert cand.ndim == 3 and cand.shape[0] == self.n and cand.shape[2] == ncols
        return cand.shape[1], cand, np.zeros((self.n, cand.shape[1]), dtype=self._ot)

    def bten2_select_set(self, which): self._ck(self._l.pepsgpu_bten2_select_set(self._h, int(which)))

    def cfg_override_slice(self, orient, num, states=None):
        """states [n][N] (extended states of one row / column read instead of the walkers' own), None: clear"""
        if states is None:
            self._ck(self._l.pepsgpu_cfg_override_slice(self._h, orient, num, None))
        else:
            st = np.ascontiguousarray(states, dtype=np.int32)
            # (the C ABI carries no length: the engine reads states[w * N + j], N = columns of a row / rows of a column)
            want = self.cols if orient == HORIZONTAL else self.rows
            assert st.ndim == 2 and st.shape[0] == self.n and st.shape[1] == want, (st.shape, self.n, want)
            self._ck(self._l.pepsgpu_cfg_override_slice(self._h, orient, num, _ip(st)))

    def replace_plaquette_trace(self, row, col, cand_states=None, left_set=0, right_set=0):
        """cand_states [n][n_cand][4]: states of (row, col), (row+1, col), (row+1, col+1), (row, col+1); None: the walkers' own"""
        nc, cand, out = self._cand(cand_states, 4)
        self._ck(self._l.pepsgpu_replace_plaquette_trace(self._h, row, col, nc, None if cand is None else _ip(cand), left_set, right_set,
                                                         _dp(out)))
        return out

    def replace_nnn_trace(self, row, col, nnn_dir, orient, cand_states=None):
        nc, cand, out = self._cand(cand_states, 2)
        self._ck(self._l.pepsgpu_replace_nnn_trace(self._h, row, col, nnn_dir, orient, nc,
                                                   None if cand is None else _ip(cand), _dp(out)))
        return out

    def replace_tnn_trace(self, row, col, orient, cand_states=None):
        nc, cand, out = self._cand(cand_states, 3)
        self._ck(self._l.pepsgpu_replace_tnn_trace(self._h, row, col, orient, nc,
                                                   None if cand is None else _ip(cand), _dp(out)))
        return out

    def replace_sqrt5_trace(self, row, col, link_dir, orient, cand_states=None):
        nc, cand, out = self._cand(cand_states, 2)
        self._ck(self._l.pepsgpu_replace_sqrt5_trace(self._h, row, col, link_dir, orient, nc,
                                                     None if cand is None else _ip(cand), _dp(out)))
        return out

    def punch_hole(self, row, col, orient):
        out = np.zeros((self.n, self.D, self.D, self.D, self.D), dtype=self._ot)
        self._ck(self._l.pepsgpu_punch_hole(self._h, row, col, orient, _dp(out)))
        return out

    def trace_scaling(self, on_device):
        """trace / replace_nn_trace / replace_one_trace multiply by exp(log-scale) in a kernel, as the device-side slices do (True), or
        with std::exp on the host (False, the default): the two may differ in the last bit"""
        self._ck(self._l.pepsgpu_trace_scaling(self._h, int(bool(on_device))))

    def punch_hole_store(self, row, col, orient):
        self._ck(self._l.pepsgpu_punch_hole(self._h, row, col, orient, None))

    # -- stochastic reconfiguration: O* samples resident in HBM --
    def sr_begin(self, max_samples):
        self._ck(self._l.pepsgpu_sr_begin(self._h, max_samples))

    def sr_append(self, psi):
        psi = np.ascontiguousarray(psi, dtype=self._ot)
        self._ck(self._l.pepsgpu_sr_append(self._h, _dp(psi)))

    def sr_count(self):
        return self._l.pepsgpu_sr_count(self._h)

    def sr_sum(self):
        out = np.zeros((self.rows, self.cols, self.d, self.D, self.D, self.D, self.D), dtype=self._ot)
        self._ck(self._l.pepsgpu_sr_sum(self._h, _dp(out)))
        return out

    def sr_matvec(self, v, mean_dot_v, scale):
        v = np.ascontiguousarray(v, dtype=self._ot)
        out = np.zeros_like(v)
        if self._ot is np.complex128:
            m = complex(mean_dot_v)
            self._ck(self._l.pepsgpu_sr_matvec_c128(self._h, _dp(v), m.real, m.imag, float(scale), _dp(out)))
        else:
            self._ck(self._l.pepsgpu_sr_matvec(self._h, _dp(v), float(mean_dot_v), float(scale), _dp(out)))
        return out

    def sr_cg_solve(self, b, x0=None, diag_shift=0.0, max_iter=100, relative_tolerance=1e-4, absolute_tolerance=0.0,
                    residual_recompute_interval=20, orthogonality_threshold=0.5):
        """(S + diag_shift) x = b with every CG vector on the device; returns (x, residual_norm, iterations, reason)."""
        dt = np.complex128 if self.dtype == C128 else np.float64       # complex contexts: interleaved (re, im) pairs through the C ABI
        b = np.ascontiguousarray(b, dtype=dt)
        x0a = None if x0 is None else np.ascontiguousarray(x0, dtype=dt)
        x = np.zeros_like(b)
        res = np.zeros(1, dtype=np.float64)
        it = np.zeros(2, dtype=np.int32)
        self._ck(self._l.pepsgpu_sr_cg_solve(self._h, _dp(b), None if x0a is None else _dp(x0a), diag_shift, max_iter,
                                             relative_tolerance, absolute_tolerance, residual_recompute_interval,
                                             orthogonality_threshold, _dp(x), _dp(res), _ip(it[:1]), _ip(it[1:])))
        return x, float(res[0]), int(it[0]), int(it[1])

    def sr_gram(self, remote_samples_ptr=None, remote_configs_ptr=None, n_remote=0):
        """raw inner products of the local O* samples with themselves (default) or with a device-resident remote batch"""
        n = self.sr_count()
        dt = np.complex128 if self.dtype == C128 else np.float64       # complex contexts: ip_ij = sum conj(O*_i) O*_j, interleaved pairs
        out = np.zeros((n, n_remote if remote_samples_ptr else n), dtype=dt)
        self._ck(self._l.pepsgpu_sr_gram(self._h, remote_samples_ptr, remote_configs_ptr, n_remote, _dp(out)))
        return out

    def sr_weighted_sum(self, y):
        dt = np.complex128 if self.dtype == C128 else np.float64
        y = np.ascontiguousarray(y, dtype=dt)
        assert y.size == self.sr_count()
        out = np.zeros((self.rows, self.cols, self.d, self.D, self.D, self.D, self.D), dtype=dt)
        self._ck(self._l.pepsgpu_sr_weighted_sum(self._h, _dp(y), _dp(out)))
        return out

    def sr_copy_samples(self, dst_samples_ptr, dst_configs_ptr):
        self._ck(self._l.pepsgpu_sr_copy_samples(self._h, dst_samples_ptr, dst_configs_ptr))

    # -- device-resident optimisation step: theta, g and the rule state stay in HBM (include/pepsgpu.h, pepsgpu_opt_*) --
    OPT_SGD, OPT_ADAGRAD, OPT_ADAM = 0, 1, 2

    def _state_shape(self):
        return (self.rows, self.cols, self.d, self.D, self.D, self.D, self.D)

    def opt_begin(self):
        self._ck(self._l.pepsgpu_opt_begin(self._h))

    def opt_end(self):
        self._ck(self._l.pepsgpu_opt_end(self._h))

    def opt_gradient_from_accumulators(self, e_loc_sum, weight_sum):
        """g <- (S_EO - conj(E) S_O) / W from the resident accumulators; returns (E, |g|)."""
        es = np.ascontiguousarray([e_loc_sum], dtype=self._ot)
        e = np.zeros(1, dtype=self._ot)
        nrm = np.zeros(1, dtype=np.float64)
        self._ck(self._l.pepsgpu_opt_gradient_from_accumulators(self._h, _dp(es), float(weight_sum), _dp(e), _dp(nrm)))
        return e[0], float(nrm[0])

    def opt_set_gradient(self, g):
        g = np.ascontiguousarray(g, dtype=self._ot)
        if g.shape != self._state_shape():
            raise ValueError("the gradient has the padded state layout %s" % (self._state_shape(),))
        self._ck(self._l.pepsgpu_opt_set_gradient(self._h, _dp(g)))

    def opt_get_gradient(self):
        out = np.zeros(self._state_shape(), dtype=self._ot)
        self._ck(self._l.pepsgpu_opt_get_gradient(self._h, _dp(out)))
        return out

    def opt_clip(self, clip_value=0.0, clip_norm=0.0):
        """element-wise clip, then global-norm clip (a bound <= 0 is off); returns |g| on entry"""
        nrm = np.zeros(1, dtype=np.float64)
        self._ck(self._l.pepsgpu_opt_clip(self._h, float(clip_value), float(clip_norm), _dp(nrm)))
        return float(nrm[0])

    def opt_natural_gradient(self, diag_shift=0.001, max_iter=100, relative_tolerance=1e-4, absolute_tolerance=0.0,
                             residual_recompute_interval=20, orthogonality_threshold=0.5):
        """g <- (S + diag_shift)^-1 g on the device; returns (residual_norm, iterations, reason, |direction|)."""
        res = np.zeros(2, dtype=np.float64)
        it = np.zeros(2, dtype=np.int32)
        self._ck(self._l.pepsgpu_opt_natural_gradient(self._h, diag_shift, max_iter, relative_tolerance, absolute_tolerance,
                                                      residual_recompute_interval, orthogonality_threshold, _dp(res[:1]),
                                                      _ip(it[:1]), _ip(it[1:]), _dp(res[1:])))
        return float(res[0]), int(it[0]), int(it[1]), float(res[1])

    def opt_step(self, rule, lr, params):
        """rule 0 SGD (momentum, nesterov, weight_decay), 1 AdaGrad (epsilon, initial_accumulator_value),
        2 Adam (beta1, beta2, epsilon, weight_decay)"""
        p = np.ascontiguousarray(params, dtype=np.float64).ravel()
        self._ck(self._l.pepsgpu_opt_step(self._h, int(rule), float(lr), _dp(p), p.size))

    def opt_scale_state(self, factor):
        self._ck(self._l.pepsgpu_opt_scale_state(self._h, float(factor)))

    def opt_read_state(self):
        out = np.zeros(self._state_shape(), dtype=self._ot)
        self._ck(self._l.pepsgpu_opt_read_state(self._h, _dp(out)))
        return out

    # -- the lowest-energy parameters of a VMC run, kept in HBM (include/pepsgpu.h, pepsgpu_vmc_snapshot_*) --
    def vmc_snapshot_save(self):
        """device-to-device copy of theta into the snapshot buffer (allocated on first use, freed by opt_end)"""
        self._ck(self._l.pepsgpu_vmc_snapshot_save(self._h))

    def vmc_snapshot_read(self):
        """the snapshot in the layout of opt_read_state"""
        out = np.zeros(self._state_shape(), dtype=self._ot)
        self._ck(self._l.pepsgpu_vmc_snapshot_read(self._h, _dp(out)))
        return out

    def vmc_snapshot_clear(self):
        self._ck(self._l.pepsgpu_vmc_snapshot_clear(self._h))

    # -- the base of a step: rollback and step-selector trials in HBM (include/pepsgpu.h, pepsgpu_guard_*) --
    def opt_base_save(self):
        """base <- theta, device to device (allocated on first use, freed by opt_end)"""
        self._ck(self._l.pepsgpu_guard_base_save(self._h))

    def opt_base_restore(self):
        """theta <- base and device state = T(base); the gradient buffer is not read"""
        self._ck(self._l.pepsgpu_guard_base_restore(self._h))

    def opt_base_clear(self):
        """no base afterwards; the buffer stays"""
        self._ck(self._l.pepsgpu_guard_base_clear(self._h))

    def opt_preview(self, rule, lr, params):
        """theta <- the SGD rule (rule 0; momentum, nesterov, weight_decay) applied to the saved base with the current g; the
        velocity is read and not written.  (0, 0, 0) is base - lr g, the trial along an SR / MinSR direction."""
        p = np.ascontiguousarray(params, dtype=np.float64).ravel()
        self._ck(self._l.pepsgpu_guard_preview(self._h, int(rule), float(lr), _dp(p), p.size))

    def minsr_direction(self, eloc, energy, r_pinv=1e-12, a_pinv=0.0, soft_cutoff=True):
        """g <- the MinSR direction of the resident sample store (Gram, centering, eigensolve, cutoff, back-substitution: all on the
        device); `eloc` = the local energies in the order of the store, `energy` = their mean.  Returns (|g|, dict with lambda_max,
        cutoff, n_kept, sweeps).  pepsgpu_opt_step with rule 0 applies it."""
        e = np.ascontiguousarray(eloc, dtype=self._ot).ravel()
        if self.sr_count() > 0 and e.size != self.sr_count():      # (an empty store is refused by the library)
            raise ValueError("one local energy per stored sample (%d), got %d" % (self.sr_count(), e.size))
        en = np.ascontiguousarray([energy], dtype=self._ot)
        nrm = np.zeros(1, dtype=np.float64)
        info = np.zeros(4, dtype=np.float64)
        self._ck(self._l.pepsgpu_minsr_direction(self._h, _dp(e), _dp(en), float(r_pinv), float(a_pinv), int(bool(soft_cutoff)),
                                                 _dp(nrm), _dp(info)))
        return float(nrm[0]), {"lambda_max": float(info[0]), "cutoff": float(info[1]), "n_kept": int(info[2]), "sweeps": int(info[3])}

    # -- L-BFGS on the optimizer buffers: history, anchor, direction and the base of the line search stay in HBM (pepsgpu_lbfgs_*) --
    LBFGS_NONE, LBFGS_PUSHED, LBFGS_PUSHED_DAMPED, LBFGS_SKIPPED = 0, 1, 2, 3

    def lbfgs_begin(self, history_size):
        self._ck(self._l.pepsgpu_lbfgs_begin(self._h, int(history_size)))

    def lbfgs_end(self):
        self._ck(self._l.pepsgpu_lbfgs_end(self._h))

    def lbfgs_reset(self):
        self._ck(self._l.pepsgpu_lbfgs_reset(self._h))

    def lbfgs_update(self, min_curvature=1e-12, use_damping=True):
        """history update from the anchor, theta and the gradient buffer; returns (outcome, curvature): 0 no anchor, 1 pushed,
        2 pushed after damping, 3 skipped"""
        oc = np.zeros(1, dtype=np.int32)
        cv = np.zeros(1, dtype=np.float64)
        self._ck(self._l.pepsgpu_lbfgs_update(self._h, float(min_curvature), int(bool(use_damping)), _ip(oc), _dp(cv)))
        return int(oc[0]), float(cv[0])

    def lbfgs_direction(self, min_curvature=1e-12, max_direction_norm=1e3):
        """d <- the two-loop direction of the gradient buffer (norm cap, descent guard), base of the search <- (theta, g); returns
        (<g,d>, |d|, was_reset)"""
        out = np.zeros(2, dtype=np.float64)
        rs = np.zeros(1, dtype=np.int32)
        self._ck(self._l.pepsgpu_lbfgs_direction(self._h, float(min_curvature), float(max_direction_norm), _dp(out[:1]), _dp(out[1:]),
                                                 _ip(rs)))
        return float(out[0]), float(out[1]), bool(rs[0])

    def lbfgs_trial(self, alpha):
        """theta = theta_base + alpha d, device state = T(theta)"""
        self._ck(self._l.pepsgpu_lbfgs_trial(self._h, float(alpha)))

    def lbfgs_slope(self):
        out = np.zeros(1, dtype=np.float64)
        self._ck(self._l.pepsgpu_lbfgs_slope(self._h, _dp(out)))
        return float(out[0])

    def lbfgs_commit(self):
        self._ck(self._l.pepsgpu_lbfgs_commit(self._h))

    def lbfgs_get_direction(self):
        out = np.zeros(self._state_shape(), dtype=self._ot)
        self._ck(self._l.pepsgpu_lbfgs_get_direction(self._h, _dp(out)))
        return out

    def lbfgs_get_pair(self, index):
        """(s, y) of pair `index` of the history, 0 = oldest"""
        s = np.zeros(self._state_shape(), dtype=self._ot)
        y = np.zeros(self._state_shape(), dtype=self._ot)
        self._ck(self._l.pepsgpu_lbfgs_get_pair(self._h, int(index), _dp(s), _dp(y)))
        return s, y

    def lbfgs_counters(self):
        out = (C.c_long * 4)()
        self._ck(self._l.pepsgpu_lbfgs_counters(self._h, out))
        return {"skip_curvature": int(out[0]), "damping": int(out[1]), "descent_reset": int(out[2]), "history": int(out[3])}

    def diag_eigh(self, a):
        """the device eigensolver alone: a real symmetric or complex Hermitian matrix -> (w ascending, z with A z[:, k] = w[k] z[:, k],
        Jacobi sweeps)"""
        cplx = np.iscomplexobj(a)
        a = np.ascontiguousarray(a, dtype=np.complex128 if cplx else np.float64)
        if a.ndim != 2 or a.shape[0] != a.shape[1]:
            raise ValueError("a square matrix")
        n = a.shape[0]
        w = np.zeros(n, dtype=np.float64)
        z = np.zeros((n, n), dtype=a.dtype)
        sw = np.zeros(1, dtype=np.int32)
        self._ck(self._l.pepsgpu_diag_eigh(self._h, n, int(cplx), _dp(a), _dp(w), _dp(z), _ip(sw)))
        return w, z, int(sw[0])

    def diag_truncate_site(self, M, u, k2, rows=None, route=0):
        """the truncation of one interior site as a row absorption of this context (F64 or C128) runs it, on given matrices
        M [nb][m][u * k2], nb <= max_walkers.  rows (F64 only): live rows of M per entry.  route: 0 the dispatch as shipped, 1 the
        round-6 form, 2 the round-5 two-Cholesky form, 3 general kernels only (1 .. 3 override the environment for this call).
        Returns V [nb][k][u * k2] with k = min(chi, m, u * k2), klive [nb] (-1 on a complex context) and route_flag [nb]
        (< 0: a dense route delivered the entry's rows, >= 0: the general kernels did)."""
        if self.dtype not in (F64, C128):
            raise ValueError("diag_truncate_site: F64 and C128 contexts only")
        t = np.complex128 if self.dtype == C128 else np.float64
        M = np.ascontiguousarray(M, dtype=t)
        nb, m, ln = M.shape
        if ln != u * k2:
            raise ValueError("M must be [nb][m][u * k2]")
        k = min(self.chi, m, ln)
        if rows is not None:
            rows = np.ascontiguousarray(rows, dtype=np.int32)
            assert rows.shape == (nb,)
        V = np.zeros((nb, k, ln), dtype=t)
        kl = np.zeros(nb, dtype=np.int32)
        fl = np.zeros(nb, dtype=np.int32)
        self._ck(self._l.pepsgpu_diag_truncate_site(self._h, M.ctypes.data_as(C.c_void_p), nb, m, int(u), int(k2),
                                                    None if rows is None else _ip(rows), int(route),
                                                    V.ctypes.data_as(C.c_void_p), _ip(kl), _ip(fl)))
        return V, kl, fl

    def fermion_decoration_set(self, state):
        """Tells the optimizer calls that the context holds the decorated components of `state` (a fermion.FermionState; the
        context's phys_dim is 4 * state.d): theta, g and the rule state stay in the extended layout and in the range of the
        decoration, norms are those of the stored parameters.  None clears the decoration.  Refused while optimizer buffers exist."""
        if state is None:
            self._ck(self._l.pepsgpu_fermion_decoration_set(self._h, 0, None, None))
            return
        nf = np.ascontiguousarray(state.nf, dtype=np.int32)
        par = np.zeros((self.rows, self.cols, 4, self.D), dtype=np.uint8)
        if (state.rows, state.cols) != (self.rows, self.cols) or state.D > self.D:
            raise ValueError("the state does not fit the context")
        for r in range(self.rows):
            for c in range(self.cols):
                for leg in range(4):
                    p = np.asarray(state.par[r][c][leg])
                    if np.any((p < 0) | (p > 255)):
                        raise ValueError("a bond parity outside {0, 1}")
                    par[r, c, leg, :len(p)] = p
        self._ck(self._l.pepsgpu_fermion_decoration_set(self._h, int(state.d), _ip(nf), par.ctypes.data_as(C.POINTER(C.c_uint8))))

    def grad_reset(self):
        self._ck(self._l.pepsgpu_grad_reset(self._h))

    def grad_accumulate(self, psi, eloc, exact_sum=False, states=None):
        """states ([n][rows][cols], optional): the component every stored hole belongs to, when it is not the walkers'
        current configuration (fermionic states: extended states of the row-major decoration)."""
        psi = np.ascontiguousarray(psi, dtype=np.float64)
        eloc = np.ascontiguousarray(eloc, dtype=np.float64)
        if states is None:
            self._ck(self._l.pepsgpu_grad_accumulate(self._h, _dp(psi), _dp(eloc), int(exact_sum)))
            return
        states = np.ascontiguousarray(states, dtype=np.int32)
        if states.shape != (len(psi), self.rows, self.cols):
            raise ValueError("states must be [n][rows][cols]")
        self._ck(self._l.pepsgpu_grad_accumulate_states(self._h, _dp(psi), _dp(eloc), int(exact_sum),
                                                        states.ctypes.data_as(C.POINTER(C.c_int32))))

    def grad_read(self):
        shp = (self.rows, self.cols, self.d, self.D, self.D, self.D, self.D)
        so, seo = np.zeros(shp), np.zeros(shp)
        self._ck(self._l.pepsgpu_grad_read(self._h, _dp(so), _dp(seo)))
        return so, seo

    # -- the exchange step: RCCL all-reduce of the accumulators (one rank = one context per GPU) --
    def grad_device_ptr(self):
        """(S_O pointer, S_EO pointer, elements): the float64 accumulators where they live in HBM."""
        so, seo, n = C.c_void_p(), C.c_void_p(), C.c_long()
        self._ck(self._l.pepsgpu_grad_device_ptr(self._h, C.byref(so), C.byref(seo), C.byref(n)))
        return so.value, seo.value, n.value

    def bcast_state(self, root=0):
        """ncclBroadcast of the flat SITPS in HBM from rank `root` over the context's communicator (comm_init)"""
        self._ck(self._l.pepsgpu_bcast_state(self._h, int(root)))

    def grad_allreduce(self):
        self._ck(self._l.pepsgpu_grad_allreduce(self._h))

    def comm_init(self, nranks, rank, unique_id=None):
        """unique_id: the 128 bytes of comm_unique_id() of rank 0 (None only for a single rank)."""
        buf = None if unique_id is None else C.create_string_buffer(bytes(unique_id), 128)
        self._ck(self._l.pepsgpu_comm_init(self._h, nranks, rank, buf))

    def comm_size(self): return self._l.pepsgpu_comm_size(self._h)
    def comm_rank(self): return self._l.pepsgpu_comm_rank(self._h)
    def comm_destroy(self): self._ck(self._l.pepsgpu_comm_destroy(self._h))

    def allreduce(self, arr, op="sum"):
        """in-place all-reduce of a host NumPy array (float32 / float64 / int32) over the context's communicator"""
        code = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.int32): 2}[arr.dtype]
        assert arr.flags["C_CONTIGUOUS"]
        self._ck(self._l.pepsgpu_allreduce(self._h, arr.ctypes.data_as(C.c_void_p), arr.size, code, {"sum": 0, "max": 1}[op], 0))
        return arr

    def allreduce_device(self, ptr, n, dtype=F64, op="sum"):
        self._ck(self._l.pepsgpu_allreduce(self._h, C.c_void_p(ptr), n, {F32: 0, F64: 1}[dtype], {"sum": 0, "max": 1}[op], 1))

    def update_local(self, sites, new_states, accept_mask=None):
        sites = np.ascontiguousarray(sites, dtype=np.int32).reshape(-1, 2)
        ns = np.ascontiguousarray(new_states, dtype=np.int32).reshape(self.n, sites.shape[0])
        m = None
        if accept_mask is not None:
            m = np.ascontiguousarray(accept_mask, dtype=np.uint8)
        self._ck(self._l.pepsgpu_update_local(self._h, sites.shape[0], _ip(sites), _ip(ns),
                                              m.ctypes.data_as(C.POINTER(C.c_uint8)) if m is not None else None))

    def erase_envs_after_update(self, row, col):
        self._ck(self._l.pepsgpu_erase_envs_after_update(self._h, row, col))

    def evaluate_amplitude(self):
        out = np.zeros(self.n, dtype=self._ot)
        self._ck(self._l.pepsgpu_evaluate_amplitude(self._h, _dp(out)))
        return out

    def walker_flags(self):
        out = np.zeros(self.n, dtype=np.int32)
        self._ck(self._l.pepsgpu_walker_flags(self._h, _ip(out)))
        return out

    def sync(self):
        self._ck(self._l.pepsgpu_sync(self._h))

    PROF_CATS = ("contract", "gram_f64", "cholesky", "jacobi", "select", "normalize", "env", "jacobi_edge", "trunc_gram",
                 "trunc_apply", "contract_chain")

    def profile_enable(self, on=True):
        self._ck(self._l.pepsgpu_profile_enable(self._h, int(on)))

    def profile_read(self):
        out = np.zeros((len(self.PROF_CATS), 5), dtype=np.float64)
        self._ck(self._l.pepsgpu_profile_read(self._h, _dp(out)))
        return {name: {"ms": out[i, 0], "launches": int(out[i, 1]), "alg_flops": out[i, 2], "exec_flops": out[i, 3],
                       "bytes": out[i, 4]}
                for i, name in enumerate(self.PROF_CATS)}

    def stats(self):
        out = np.zeros(9, dtype=np.float64)
        self._ck(self._l.pepsgpu_stats(self._h, _dp(out), 9))
        return {"absorptions": int(out[0]), "jacobi_launches": int(out[1]), "jacobi_sweeps_sum": int(out[2]),
                "device_bytes": int(out[3]), "jacobi_sweeps_max": int(out[4]),
                "carry_live_fraction": float(out[5] / out[6]) if out[6] > 0 else None,
                "carry_live_max": int(out[7]), "absorptions_redone": int(out[8])}


def comm_unique_id():
    """ncclGetUniqueId through the library: 128 bytes that rank 0 hands to every rank (MPI_Bcast in the reference host,
    torch.distributed.broadcast_object_list in peps_amd/dist.py)."""
    buf = C.create_string_buffer(128)
    rc = lib().pepsgpu_comm_unique_id(buf)
    if rc != 0:
        raise RuntimeError("pepsgpu_comm_unique_id failed: %s" % lib().pepsgpu_last_error(None).decode())
    return buf.raw


# -- diagnostics (kernel unit tests) --
def diag_tgemm(dtype_in, dtype_out, I, J, K, sAi, sAk, sBk, sBj, sCi, sCj, A, B, C_init, nbatch, wA, wB, wC):
    ints = np.array(list(I) + list(J) + list(K) + list(sAi) + list(sAk) + list(sBk) + list(sBj) + list(sCi) + list(sCj),
                    dtype=np.int32)
    tin = np.float32 if dtype_in == F32 else np.float64
    tout = np.float32 if dtype_out == F32 else np.float64
    A = np.ascontiguousarray(A, dtype=tin)
    B = np.ascontiguousarray(B, dtype=tin)
    Cc = np.ascontiguousarray(C_init, dtype=tout).copy()
    rc = lib().pepsgpu_diag_tgemm(dtype_in, dtype_out, _ip(ints), 27, A.ctypes.data_as(C.c_void_p), A.size,
                                  B.ctypes.data_as(C.c_void_p), B.size, Cc.ctypes.data_as(C.c_void_p), Cc.size,
                                  nbatch, wA, wB, wC)
    if rc != 0:
        raise RuntimeError("diag_tgemm failed: %s" % lib().pepsgpu_last_error(None).decode())
    return Cc


# element types of pepsgpu_diag_tgemm_desc: (A, B, C, accumulation)
TG_F32, TG_F32_ACC64, TG_F32_TO_F64, TG_F64, TG_C128 = 0, 1, 2, 3, 4
TG_TYPES = {TG_F32: (np.float32, np.float32, np.float32, np.float32), TG_F32_ACC64: (np.float32, np.float32, np.float32, np.float64),
            TG_F32_TO_F64: (np.float32, np.float32, np.float64, np.float64), TG_F64: (np.float64,) * 4,
            TG_C128: (np.complex128,) * 4}
# tgemm.h TgRouteKind
TG_ROUTE_EMPTY, TG_ROUTE_DIRECT, TG_ROUTE_SKINNY_128x32, TG_ROUTE_SKINNY_32x128, TG_ROUTE_TILED_MFMA, TG_ROUTE_TILED_VALU, \
    TG_ROUTE_REFUSED = range(7)
_DYN = ("dI0", "dI1", "dI2", "dJ0", "dJ1", "dJ2", "dK0", "dK1", "dK2")


def tgemm_desc_arrays(desc):
    """Flat (ints, longs, doubles, pool) of a descriptor given as a dict (keys as the TGemmDesc fields; a per-batch array is
    a sequence of ints; the TgDyn fields as desc["dI1"] = dict(p=..., mul=1, mask=0, div=1))."""
    pool = []

    def off(a):
        if a is None:
            return -1
        o = len(pool)
        pool.extend(int(v) for v in np.asarray(a).ravel())
        return o

    g = desc.get
    ints = [0] * 89
    for q, key in enumerate(("I", "J", "K", "sAi", "sAk", "sBk", "sBj", "sCi", "sCj")):
        dflt = (1, 1, 1) if q < 3 else (0, 0, 0)
        ints[3 * q:3 * q + 3] = [int(v) for v in g(key, dflt)]
    for q, key in enumerate(_DYN):
        t = g(key) or {}
        ints[27 + q] = off(t.get("p"))
        ints[36 + q] = int(t.get("mul", 1))
        ints[45 + q] = int(t.get("mask", 0))
        ints[54 + q] = int(t.get("div", 1))
    ints[63], ints[64] = off(g("dynI")), off(g("dynK"))
    ints[65], ints[66] = int(g("dynI_mul", 1)), int(g("dynK_mul", 1))
    ints[67], ints[68] = off(g("selA")), off(g("selB"))
    ints[69], ints[70] = int(g("selA_inc", 0)), int(g("selB_inc", 0))
    ints[71:76] = [int(g(k, 1)) for k in ("bdivA", "bdivB", "bdivC", "seldivA", "seldivB")]
    ints[76] = int(g("nbatch", 1))
    ints[77:81] = [int(g(k, 0)) for k in ("accumulate", "upper_only", "conjA", "conjB")]
    ints[81] = off(g("batch_flag"))
    ints[82], ints[83] = int(g("prefer_tiled", 0)), int(g("acc64", 0))
    ints[84:88] = [int(bool(g(k, False))) for k in ("scale_out", "norm_log", "norm_flag", "scale_in")]
    longs = [int(g(k, 0)) for k in ("wA", "wB", "wC", "selA_mul", "selB_mul")]
    return (np.array(ints, dtype=np.int32), np.array(longs, dtype=np.int64), np.array([float(g("alpha", 1.0))]),
            np.array(pool if pool else [0], dtype=np.int32))


def diag_tnn3_table(phys_dim):
    """the bosonic triple table [phys_dim^3][20] pepsgpu_sweep_slice_tnn3 builds for a NULL table; no device is touched"""
    out = np.zeros((phys_dim ** 3, 20), dtype=np.int32)
    if lib().pepsgpu_diag_tnn3_table(phys_dim, _ip(out)) != 0:
        raise ValueError("diag_tnn3_table: 1 <= phys_dim <= 64")
    return out


def diag_tgemm_route(types, desc, a_offset=0, b_offset=0):
    """(route, avec, bvec, acc64) tgemm_launch takes for the descriptor; no device is touched."""
    ints, longs, dbls, _ = tgemm_desc_arrays(desc)
    r = np.zeros(4, dtype=np.int32)
    rc = lib().pepsgpu_diag_tgemm_route(types, _ip(ints), ints.size, longs.ctypes.data_as(C.POINTER(C.c_long)), longs.size,
                                        _dp(dbls), dbls.size, a_offset, b_offset, _ip(r))
    if rc != 0:
        raise RuntimeError("diag_tgemm_route failed: %s" % lib().pepsgpu_last_error(None).decode())
    return tuple(int(v) for v in r)


def diag_tgemm_desc(types, desc, A, B, C_init, a_offset=0, b_offset=0, scale_in=None, scale_out=None, norm_log=None,
                    norm_flag=None):
    """One tgemm_launch of the descriptor (see tgemm_desc_arrays) on flat operand buffers; A is read from A[a_offset:], B from
    B[b_offset:].  scale_in: per-entry input scales (desc["scale_in"] set); scale_out / norm_log / norm_flag: initial values of
    the outputs the descriptor enables.  Returns a dict: status (0 or the library's error code), C, route (route, avec, bvec,
    acc64), flops, scale_out, norm_log, norm_flag."""
    ints, longs, dbls, pool = tgemm_desc_arrays(desc)
    ta, tb, tc, _ = TG_TYPES[types]
    nb = int(ints[76])
    A = np.ascontiguousarray(A, dtype=ta)
    B = np.ascontiguousarray(B, dtype=tb)
    Cc = np.ascontiguousarray(C_init, dtype=tc).copy()
    si = np.ascontiguousarray(np.ones(max(nb, 1)) if scale_in is None else scale_in, dtype=np.float32)
    so = np.ascontiguousarray(np.zeros(max(nb, 1)) if scale_out is None else scale_out, dtype=np.float32).copy()
    nl = np.ascontiguousarray(np.zeros(max(nb, 1)) if norm_log is None else norm_log, dtype=np.float64).copy()
    nf = np.ascontiguousarray(np.zeros(max(nb, 1)) if norm_flag is None else norm_flag, dtype=np.int32).copy()
    route = np.full(4, -1, dtype=np.int32)
    flops = C.c_ulonglong(0)
    fp = C.POINTER(C.c_float)
    rc = lib().pepsgpu_diag_tgemm_desc(types, _ip(ints), ints.size, longs.ctypes.data_as(C.POINTER(C.c_long)), longs.size,
                                       _dp(dbls), dbls.size, _ip(pool), pool.size, si.ctypes.data_as(fp),
                                       A.ctypes.data_as(C.c_void_p), A.size, a_offset, B.ctypes.data_as(C.c_void_p), B.size, b_offset,
                                       Cc.ctypes.data_as(C.c_void_p), Cc.size, so.ctypes.data_as(fp), _dp(nl), _ip(nf), _ip(route),
                                       C.byref(flops))
    return dict(status=int(rc), C=Cc, route=tuple(int(v) for v in route), flops=int(flops.value), scale_out=so, norm_log=nl,
                norm_flag=nf, error=lib().pepsgpu_last_error(None).decode() if rc else "")


def diag_tgemm_chain3(dims, site_strides, site, slot, sel, sel_inc, mps1, bten, mps2, out_init, live=None, skip=None, offs=(0, 0, 0)):
    """One BTen growth step through tgemm_chain3_kernel with the engine's descriptors (bten_chain_descs).  dims = (x, p1, cdim,
    b1, b2, s1, s2, y); site = flat store of slot-element tensors (legs p1, b1, s1, s2 at site_strides), entry b uses tensor
    sel[b * sel_inc]; mps1 / bten / mps2 = flat per-entry buffers, offs = element offsets of the mps1 / bten / site bases in
    theirs; live = per entry (vx, vc, vb, vy) or None; out_init = the initial output.  Returns (out, flags, launched, variant)."""
    d8 = np.ascontiguousarray(dims, dtype=np.int32)
    st = np.ascontiguousarray(site_strides, dtype=np.int32)
    sel = np.ascontiguousarray(sel, dtype=np.int32)
    nb = int(np.asarray(out_init).shape[0])
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32).ravel()   # noqa: E731
    m1, bt, sv, m2 = f32(mps1), f32(bten), f32(site), f32(mps2)
    out = np.ascontiguousarray(out_init, dtype=np.float32).copy()
    lv = None if live is None else np.ascontiguousarray(live, dtype=np.int32)
    sk = None if skip is None else np.ascontiguousarray(skip, dtype=np.int32)
    o3 = np.ascontiguousarray(offs, dtype=np.int32)
    x, p1, c, b1, b2, s1, _, y = (int(v) for v in d8)
    for buf, n, o in ((m1, x * p1 * c, o3[0]), (bt, c * b1 * b2, o3[1]), (m2, b2 * s1 * y, 0)):
        if buf.size != n * nb + o:
            raise ValueError("diag_tgemm_chain3: operand buffer of %d elements, expected %d" % (buf.size, n * nb + o))
    if sel.size < (nb - 1) * sel_inc + 1 or (sv.size - int(o3[2])) < slot * (int(sel.max()) + 1):
        raise ValueError("diag_tgemm_chain3: selector or site store too small")
    flags = np.full(nb, 7, dtype=np.int32)
    launched = np.zeros(1, dtype=np.int32)
    variant = np.zeros(3, dtype=np.int32)
    vpp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    rc = lib().pepsgpu_diag_tgemm_chain3(_ip(d8), _ip(st), slot, (sv.size - int(offs[2])) // slot, _ip(sel), sel_inc,
                                         None if lv is None else _ip(lv), None if sk is None else _ip(sk), nb, _ip(o3),
                                         vpp(m1), vpp(bt), vpp(sv), vpp(m2), vpp(out), _ip(flags), _ip(launched), _ip(variant))
    if rc != 0:
        raise RuntimeError("diag_tgemm_chain3 failed: %s" % lib().pepsgpu_last_error(None).decode())
    return out, flags, int(launched[0]), tuple(int(v) for v in variant)


def diag_tgemm_chain(R, A, W, live):
    """P[b][m,u,l2,a2] = sum R[b][m,l,a] A[b][a,p,a2] W[b][l,p,l2,u] over the live extents live[b] = (m, a, a2), through
    tgemm_chain_kernel with the descriptors of Engine::absorb_impl; returns (P, flags)."""
    R = np.ascontiguousarray(R, dtype=np.float32); A = np.ascontiguousarray(A, dtype=np.float32)
    W = np.ascontiguousarray(W, dtype=np.float32)
    nb, m, l, a = R.shape
    _, _, p, a2 = A.shape
    l2, u = W.shape[3], W.shape[4]
    dims = np.array([m, l, a, p, a2, l2, u], dtype=np.int32)
    lv = np.ascontiguousarray(live, dtype=np.int32)
    P = np.zeros((nb, m, u, l2, a2), dtype=np.float32)
    fl = np.zeros(nb, dtype=np.int32)
    f = lib().pepsgpu_diag_tgemm_chain
    f.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
    rc = f(_ip(dims), _ip(lv), nb, R.ctypes.data_as(C.c_void_p), A.ctypes.data_as(C.c_void_p), W.ctypes.data_as(C.c_void_p),
           P.ctypes.data_as(C.c_void_p), _ip(fl))
    if rc != 0:
        raise RuntimeError("diag_tgemm_chain failed: %s" % lib().pepsgpu_last_error(None).decode())
    return P, fl


def diag_tgemm_chain_pair(backward, dims, site_strides, site, slot, sel, op1, op2, live, out_init, d8=True, tsw=False,
                          zero_fill=False, f64=False, scale_in=None):
    """The forward pair P = W (R A) (backward False: op1 = R [nb, m, l, a], op2 = A [nb, a, p, a2], live = per entry (m, a, a2),
    out = P [nb, m, u, l2, a2]) or the backward pair Tt = W (A Y) (True: op1 = A, op2 = Y [nb, l2, a2, k2], live = (a, a2, k2),
    out = Tt [nb, l, a, u, k2], [nb, l, a, k2, u] with tsw) with the engine's descriptors.  dims = (m, a, a2, k2, l, p, l2, u);
    site = flat store of slot-element site tensors with the legs (l, p, l2, u) at site_strides, entry b uses tensor sel[b].
    d8 asks for the leg-8 kernel where its contract holds, else the generic chained kernel runs.
    Returns (out, flags, launched, ran_d8)."""
    d8v = np.ascontiguousarray(dims, dtype=np.int32)
    st = np.ascontiguousarray(site_strides, dtype=np.int32)
    sel = np.ascontiguousarray(sel, dtype=np.int32)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32).ravel()   # noqa: E731
    o1, o2, sv = f32(op1), f32(op2), f32(site)
    out = np.ascontiguousarray(out_init, dtype=np.float32).copy()
    nb = int(out.shape[0])
    lv = np.ascontiguousarray(live, dtype=np.int32)
    m, a, a2, k2, l, p, l2, u = (int(v) for v in d8v)
    n1, n2, no = ((a * p * a2, l2 * a2 * k2, l * a * u * k2) if backward else (m * l * a, a * p * a2, m * u * l2 * a2))
    if o1.size != n1 * nb or o2.size != n2 * nb or out.size != no * nb or lv.size != 3 * nb or sel.size != nb or d8v.size != 8:
        raise ValueError("diag_tgemm_chain_pair: operand sizes do not match dims")
    if sv.size % slot or int(sel.min()) < 0 or (int(sel.max()) + 1) * slot > sv.size:
        raise ValueError("diag_tgemm_chain_pair: selector or site store too small")
    reach = sum((e - 1) * int(s) for e, s in zip((l, p, l2, u), st))
    if reach >= slot or int(st.min()) < 0:
        raise ValueError("diag_tgemm_chain_pair: site strides reach beyond a slot")
    sc = None if scale_in is None else np.ascontiguousarray(scale_in, dtype=np.float32)
    flags = np.full(nb, 7, dtype=np.int32)
    info = np.zeros(2, dtype=np.int32)
    vpp = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731
    f = lib().pepsgpu_diag_tgemm_chain_pair
    f.argtypes = [C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_long, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                  C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32),
                  C.POINTER(C.c_int32)]
    opts = (1 if d8 else 0) | (2 if tsw else 0) | (4 if zero_fill else 0) | (8 if f64 else 0)
    rc = f(1 if backward else 0, _ip(d8v), _ip(st), slot, sv.size // slot, _ip(sel), _ip(lv), nb, opts,
           None if sc is None else vpp(sc), vpp(o1), vpp(o2), vpp(sv), vpp(out), _ip(flags), _ip(info))
    if rc != 0:
        raise RuntimeError("diag_tgemm_chain_pair failed: %s" % lib().pepsgpu_last_error(None).decode())
    return out, flags, int(info[0]), bool(info[1])


def diag_chain_d8_launches():
    """Launches of the leg-8 chained-pair kernel by this process."""
    f = lib().pepsgpu_diag_chain_d8_launches
    f.argtypes = []
    f.restype = C.c_long
    return int(f())


def diag_chain_d8_stats():
    """(walkers the leg-8 kernel computed, of them walked in chunks) under PEPSGPU_CHAIN_D8_STATS=1; zeros when it is unset."""
    out = (C.c_ulonglong * 2)()
    f = lib().pepsgpu_diag_chain_d8_stats
    f.argtypes = [C.POINTER(C.c_ulonglong)]
    if f(out) != 0:
        raise RuntimeError("diag_chain_d8_stats failed: %s" % lib().pepsgpu_last_error(None).decode())
    return int(out[0]), int(out[1])


def diag_chol(dtype_out, G):
    G = np.ascontiguousarray(G, dtype=np.float64)
    nb, n, _ = G.shape
    R = np.zeros((nb, n, n), dtype=np.float32 if dtype_out == F32 else np.float64)
    rc = lib().pepsgpu_diag_chol(dtype_out, _dp(G), n, nb, R.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise RuntimeError("diag_chol failed: %s" % lib().pepsgpu_last_error(None).decode())
    return R


def diag_chol_adaptive(dtype_out, G):
    """Low-rank + blocked Cholesky pair as the absorption runs it; returns (R, mlive)."""
    G = np.ascontiguousarray(G, dtype=np.float64)
    nb, n, _ = G.shape
    R = np.zeros((nb, n, n), dtype=np.float32 if dtype_out == F32 else np.float64)
    ml = np.zeros(nb, dtype=np.int32)
    rc = lib().pepsgpu_diag_chol_adaptive(dtype_out, _dp(G), n, nb, R.ctypes.data_as(C.c_void_p), _ip(ml))
    if rc != 0:
        raise RuntimeError("diag_chol_adaptive failed: %s" % lib().pepsgpu_last_error(None).decode())
    return R, ml


def diag_gram_chol(dtype, P):
    """gram_chol_lowrank_kernel alone; P = [nb][K][n]; returns (R [nb][n][n], mlive)."""
    t = np.float32 if dtype == F32 else np.float64
    P = np.ascontiguousarray(P, dtype=t)
    nb, K, n = P.shape
    R = np.zeros((nb, n, n), dtype=t)
    ml = np.zeros(nb, dtype=np.int32)
    rc = lib().pepsgpu_diag_gram_chol(dtype, P.ctypes.data_as(C.c_void_p), K, n, nb, R.ctypes.data_as(C.c_void_p), _ip(ml))
    if rc != 0:
        raise RuntimeError("diag_gram_chol failed: %s" % lib().pepsgpu_last_error(None).decode())
    return R, ml


def diag_gram_chol_wave(P, klive, inner=1, inner_live=None, max_pass=3, form=1, fill=0.0):
    """One of the two one-wave factor kernels alone (form 0: gram_chol_wave_kernel, 1: gram_chol_wave_split_kernel), then the
    list kernel for the walkers it hands on; P = [nb][K][n] float32, klive[b] live rows, inner_live[b] (optional) live inner
    indices of the (outer, inner) columns; returns (R [nb][n][n] float32, `fill` where nothing was stored, mlive)."""
    P = np.ascontiguousarray(P, dtype=np.float32)
    nb, K, n = P.shape
    kl = np.ascontiguousarray(klive, dtype=np.int32)
    il = None if inner_live is None else np.ascontiguousarray(inner_live, dtype=np.int32)
    assert kl.shape == (nb,) and (il is None or il.shape == (nb,))
    R = np.full((nb, n, n), fill, dtype=np.float32)
    ml = np.zeros(nb, dtype=np.int32)
    f = lib().pepsgpu_diag_gram_chol_wave
    fp = C.POINTER(C.c_float)
    f.argtypes = [fp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int, fp,
                  C.POINTER(C.c_int32)]
    rc = f(P.ctypes.data_as(fp), K, n, nb, _ip(kl), inner, None if il is None else _ip(il), max_pass, form, R.ctypes.data_as(fp), _ip(ml))
    if rc != 0:
        raise RuntimeError("diag_gram_chol_wave failed: %s" % lib().pepsgpu_last_error(None).decode())
    return R, ml


def diag_gram_cols(dtype, P, klive=None):
    """gram_cols_f64_kernel alone; P = [nb][K][n]; returns G [nb][n][n] float64 (64 x 64 blocks on / above the diagonal)."""
    t = np.float32 if dtype == F32 else np.float64
    P = np.ascontiguousarray(P, dtype=t)
    nb, K, n = P.shape
    G = np.zeros((nb, n, n), dtype=np.float64)
    kl = None if klive is None else np.ascontiguousarray(klive, dtype=np.int32)
    f = lib().pepsgpu_diag_gram_cols
    f.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    rc = f(dtype, P.ctypes.data_as(C.c_void_p), K, n, nb, None if kl is None else _ip(kl), _dp(G))
    if rc != 0:
        raise RuntimeError("diag_gram_cols failed: %s" % lib().pepsgpu_last_error(None).decode())
    return G


def diag_gram_rows(M, nrows):
    """gram_rows_f64_kernel alone; M = [nb][n][K] float32 (K a multiple of 16), nrows[b] live rows; returns G [nb][n][n] float64
    (64 x 64 blocks on / above the diagonal of the live part)."""
    M = np.ascontiguousarray(M, dtype=np.float32)
    nb, n, K = M.shape
    G = np.zeros((nb, n, n), dtype=np.float64)
    nr = np.ascontiguousarray(nrows, dtype=np.int32)
    f = lib().pepsgpu_diag_gram_rows
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    rc = f(M.ctypes.data_as(C.c_void_p), n, K, nb, _ip(nr), _dp(G))
    if rc != 0:
        raise RuntimeError("diag_gram_rows failed: %s" % lib().pepsgpu_last_error(None).decode())
    return G


def diag_lds_gram_chol(which, X, nlive):
    """mid_gram_chol_kernel (which = 0: X [nb][n][K], R^T R = X X^T over the nlive[b] first rows) or colgram_dense_kernel (which = 1:
    X [nb][K][n], R^T R = X^T X over the nlive[b] first rows) alone; returns (R [nb][n][n] float32 -- rows beyond mlive are NaN --, mlive)."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    nb = X.shape[0]
    n, K = (X.shape[1], X.shape[2]) if which == 0 else (X.shape[2], X.shape[1])
    R = np.zeros((nb, n, n), dtype=np.float32)
    ml = np.zeros(nb, dtype=np.int32)
    nl = np.ascontiguousarray(nlive, dtype=np.int32)
    f = lib().pepsgpu_diag_lds_gram_chol
    f.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_void_p, C.POINTER(C.c_int32)]
    rc = f(which, X.ctypes.data_as(C.c_void_p), n, K, nb, _ip(nl), R.ctypes.data_as(C.c_void_p), _ip(ml))
    if rc != 0:
        raise RuntimeError("diag_lds_gram_chol failed: %s" % lib().pepsgpu_last_error(None).decode())
    return R, ml


def diag_chol_pivot(X, nlive, kcap=64):
    """The first compression of the dense truncation route (round 6): i8 row Gram with both triangles + chol_pivot_kernel.
    X [nb][n][K] float32, 128 < n <= 256; returns (R [nb][kcap][n] float32 in pivot order -- rows beyond mlive are NaN --, mlive)."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    nb, n, K = X.shape
    R = np.zeros((nb, kcap, n), dtype=np.float32)
    ml = np.zeros(nb, dtype=np.int32)
    nl = np.ascontiguousarray(nlive, dtype=np.int32)
    f = lib().pepsgpu_diag_chol_pivot
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_void_p, C.POINTER(C.c_int32)]
    rc = f(X.ctypes.data_as(C.c_void_p), n, K, nb, _ip(nl), kcap, R.ctypes.data_as(C.c_void_p), _ip(ml))
    if rc != 0:
        raise RuntimeError("diag_chol_pivot failed: %s" % lib().pepsgpu_last_error(None).decode())
    return R, ml


def diag_rows_qr(X, klive):
    """rows_qr_kernel alone: X [nb][k][len] float32 -> (V [nb][k][len] orthonormal live rows first, klive_out)."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    nb, k, ln = X.shape
    V = np.zeros_like(X)
    ml = np.zeros(nb, dtype=np.int32)
    kl = np.ascontiguousarray(klive, dtype=np.int32)
    f = lib().pepsgpu_diag_rows_qr
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_void_p, C.POINTER(C.c_int32)]
    rc = f(X.ctypes.data_as(C.c_void_p), k, ln, nb, _ip(kl), V.ctypes.data_as(C.c_void_p), _ip(ml))
    if rc != 0:
        raise RuntimeError("diag_rows_qr failed: %s" % lib().pepsgpu_last_error(None).decode())
    return V, ml


def diag_suwa_todo(weights, init, words):
    """the device's SuwaTodoStateUpdate: a chain of len(words) / 2 updates; words = raw uint32 outputs of std::mt19937"""
    w = np.ascontiguousarray(weights, dtype=np.float64)
    wd = np.ascontiguousarray(words, dtype=np.uint32)
    steps = len(wd) // 2
    out = np.zeros(steps, dtype=np.int32)
    f = lib().pepsgpu_diag_suwa_todo
    f.argtypes = [C.POINTER(C.c_double), C.c_int, C.c_int, C.POINTER(C.c_uint32), C.c_int, C.POINTER(C.c_int32)]
    rc = f(_dp(w), len(w), int(init), wd.ctypes.data_as(C.POINTER(C.c_uint32)), steps, _ip(out))
    if rc != 0:
        raise RuntimeError("diag_suwa_todo failed: %s" % lib().pepsgpu_last_error(None).decode())
    return out


def diag_nnn_hop_slice_calls():
    """completed pepsgpu_nnn_hop_slice_fermion calls of this process"""
    return int(lib().pepsgpu_diag_nnn_hop_slice_calls())


def diag_fermion_hop_cand(ext, nf, row1, col1):
    """nnn_hop_cand_kernel alone: ext [n][rows][cols] extended row-major configurations, nf [d]; returns (cand [n][2][4], sign [n][2],
    flag [n][2]) of the plaquette (row1, col1), entry 0 LEFTUP_TO_RIGHTDOWN, entry 1 LEFTDOWN_TO_RIGHTUP"""
    e = np.ascontiguousarray(ext, dtype=np.int32)
    occ = np.ascontiguousarray(nf, dtype=np.int32)
    n, rows, cols = e.shape
    cand, sign, flag = np.zeros((n, 2, 4), dtype=np.int32), np.zeros((n, 2), dtype=np.int32), np.zeros((n, 2), dtype=np.int32)
    rc = lib().pepsgpu_diag_fermion_hop_cand(rows, cols, occ.size, _ip(occ), n, _ip(e), row1, col1, _ip(cand), _ip(sign), _ip(flag))
    if rc != 0:
        raise ValueError("diag_fermion_hop_cand: status %d" % rc)
    return cand, sign, flag


def diag_pair_slice_calls():
    """completed pepsgpu_nn_pair_slice_fermion calls of this process"""
    return int(lib().pepsgpu_diag_pair_slice_calls())


def diag_pair_cand(ext, nf, pair_table, orientation, site1, site2):
    """pair_cand_kernel alone: ext [n][rows][cols] extended configurations of the mode order of `orientation`, nf [d], pair_table
    [d * d][2][2]; (site1, site2) the flat row-major indices of the bond's left / upper and right / lower site.  Returns
    (cand [n][2][2], sign [n][2])"""
    e = np.ascontiguousarray(ext, dtype=np.int32)
    occ = np.ascontiguousarray(nf, dtype=np.int32)
    tab = np.ascontiguousarray(pair_table, dtype=np.int32)
    n, rows, cols = e.shape
    cand, sign = np.zeros((n, 2, 2), dtype=np.int32), np.zeros((n, 2), dtype=np.int32)
    rc = lib().pepsgpu_diag_pair_cand(rows, cols, occ.size, _ip(occ), _ip(tab), n, _ip(e), orientation, site1, site2, _ip(cand), _ip(sign))
    if rc != 0:
        raise ValueError("diag_pair_cand: status %d" % rc)
    return cand, sign


def diag_hop_slice_calls():
    """completed pepsgpu_nn_hop_slice_fermion calls of this process"""
    return int(lib().pepsgpu_diag_hop_slice_calls())


def diag_sector_slice_calls():
    """completed pepsgpu_sweep_slice_sector calls of this process"""
    return int(lib().pepsgpu_diag_sector_slice_calls())


def diag_sector_cand(cfg, sector_table, orientation, site1, site2, nf=None):
    """sector_cand_kernel alone: cfg [n][rows][cols] (nf given: extended configurations of the mode order of `orientation`; None: bosonic
    states), sector_table [d * d][2 + 2 max_cand]; (site1, site2) the flat row-major indices of the bond's left / upper and right / lower
    site.  Returns (cand [n][max_cand][2], meta [n][2] = (m, init))"""
    e = np.ascontiguousarray(cfg, dtype=np.int32)
    tab = np.ascontiguousarray(sector_table, dtype=np.int32)
    occ = None if nf is None else np.ascontiguousarray(nf, dtype=np.int32)
    n, rows, cols = e.shape
    max_cand = (tab.shape[1] - 2) // 2
    d = int(round(np.sqrt(tab.shape[0])))
    assert tab.ndim == 2 and d * d == tab.shape[0] and (occ is None or occ.size == d), tab.shape
    cand, meta = np.zeros((n, max_cand, 2), dtype=np.int32), np.zeros((n, 2), dtype=np.int32)
    rc = lib().pepsgpu_diag_sector_cand(rows, cols, d, None if occ is None else _ip(occ), max_cand, _ip(tab), n, _ip(e), orientation,
                                        site1, site2, _ip(cand), _ip(meta))
    if rc != 0:
        raise ValueError("diag_sector_cand: status %d" % rc)
    return cand, meta


def diag_link_slice_calls():
    """completed pepsgpu_link_exchange_slice calls of this process"""
    return int(lib().pepsgpu_diag_link_slice_calls())


def diag_link_cand(cfgs, d, orient, row1, col1):
    """corner_exchange_cand_kernel alone: cfgs [n][rows][cols] states in [0, d); returns (cand [n][2][4], flag [n][2]) of the 2 x 3
    (HORIZONTAL) or 3 x 2 (VERTICAL) window at (row1, col1): the corner states (upper-left, lower-left, lower-right, upper-right) with
    the ends of link kind 2 (entry 0) and kind 3 (entry 1) exchanged, flag -1 where the ends differ else 1"""
    c = np.ascontiguousarray(cfgs, dtype=np.int32)
    n, rows, cols = c.shape
    cand, flag = np.zeros((n, 2, 4), dtype=np.int32), np.zeros((n, 2), dtype=np.int32)
    rc = lib().pepsgpu_diag_link_cand(rows, cols, int(d), n, _ip(c), orient, row1, col1, _ip(cand), _ip(flag))
    if rc != 0:
        raise ValueError("diag_link_cand: status %d" % rc)
    return cand, flag


def diag_walker_slice_calls():
    """completed pepsgpu_walker_trace_slice calls of this process"""
    return int(lib().pepsgpu_diag_walker_slice_calls())


def diag_walker_pair_slice_calls():
    """completed pepsgpu_walker_pair_trace_slice calls of this process"""
    return int(lib().pepsgpu_diag_walker_pair_slice_calls())


def diag_walker_pair_cand(ext_rows, nf, pair_table, col, slot=0, mask=None):
    """walker_pair_cand_kernel and walker_excite_pair_kernel alone: ext_rows [n][cols] extended states of the row-major order, nf [d],
    pair_table [d * d][2][2], the pair (col, col + 1).  Returns (cand [n][2][2] (slot, site), skip [2][n], sign [n][2],
    patched [n][cols] = the rows after the patch of `slot`)"""
    e = np.ascontiguousarray(ext_rows, dtype=np.int32)
    occ = np.ascontiguousarray(nf, dtype=np.int32)
    tab = np.ascontiguousarray(pair_table, dtype=np.int32)
    n, cols = e.shape
    mk = None if mask is None else np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
    cand, skip = np.zeros((n, 2, 2), dtype=np.int32), np.zeros((2, n), dtype=np.int32)
    sign, patched = np.zeros((n, 2), dtype=np.int32), np.zeros((n, cols), dtype=np.int32)
    rc = lib().pepsgpu_diag_walker_pair_cand(cols, occ.size, _ip(occ), _ip(tab), n, _ip(e), col, slot,
                                             None if mk is None else mk.ctypes.data_as(C.POINTER(C.c_uint8)), _ip(cand), _ip(skip),
                                             _ip(sign), _ip(patched))
    if rc != 0:
        raise ValueError("diag_walker_pair_cand: status %d" % rc)
    return cand, skip, sign, patched


def diag_nnn_slice_calls():
    """completed pepsgpu_nnn_exchange_slice calls of this process"""
    return int(lib().pepsgpu_diag_nnn_slice_calls())


def diag_dot4(a, b, lsum, flag=None):
    """trace_dot4_kernel alone: a [nb][I][J][K][L], b [nb][L][K][J][I] (float32, float64 or complex128) ->
    out[e] = exp(lsum[e]) sum a[e][i][j][k][l] b[e][l][k][j][i]; entries with flag[e] >= 0 are skipped and come back as 0"""
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b, dtype=a.dtype)
    dtype = {np.dtype(np.float32): F32, np.dtype(np.float64): F64, np.dtype(np.complex128): C128}[a.dtype]
    nb = a.shape[0]
    dims = np.ascontiguousarray(a.shape[1:], dtype=np.int32)
    assert dims.size == 4 and b.shape == (nb,) + tuple(int(x) for x in dims[::-1]), (a.shape, b.shape)
    ls = np.ascontiguousarray(lsum, dtype=np.float64)
    assert ls.shape == (nb,)
    fl = None if flag is None else np.ascontiguousarray(flag, dtype=np.int32)
    out = np.zeros(nb, dtype=np.complex128 if dtype == C128 else np.float64)
    rc = lib().pepsgpu_diag_dot4(dtype, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), _ip(dims), nb, _dp(ls),
                                 None if fl is None else _ip(fl), _dp(out))
    if rc != 0:
        raise RuntimeError("diag_dot4 failed: %s" % lib().pepsgpu_last_error(None).decode())
    return out


def diag_mgemm_dense(R, Tt, a_dim, u_dim, k2_dim, tt_u_inner, m_live=None, a_live=None, k2_live=None):
    """mgemm_dense_kernel alone: R [nb][m][la], Tt [nb][la][u * k2] (inner order (u, k2), or (k2, u) with tt_u_inner) -> M [nb][m][u * k2]
    (rows beyond m_live[b] come back as NaN: untouched)."""
    R = np.ascontiguousarray(R, dtype=np.float32)
    Tt = np.ascontiguousarray(Tt, dtype=np.float32)
    nb, m, la = R.shape
    uk = u_dim * k2_dim
    assert Tt.shape == (nb, la, uk)
    M = np.zeros((nb, m, uk), dtype=np.float32)
    arrs = [None if x is None else np.ascontiguousarray(x, dtype=np.int32) for x in (m_live, a_live, k2_live)]
    f = lib().pepsgpu_diag_mgemm_dense
    ip = C.POINTER(C.c_int32)
    f.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 7 + [ip, ip, ip, C.c_void_p]
    rc = f(R.ctypes.data_as(C.c_void_p), Tt.ctypes.data_as(C.c_void_p), m, la, a_dim, u_dim, k2_dim, int(tt_u_inner), nb,
           *[None if a is None else _ip(a) for a in arrs], M.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise RuntimeError("diag_mgemm_dense failed: %s" % lib().pepsgpu_last_error(None).decode())
    return M


def diag_jacobi(dtype, M, k, force_global=False):
    """the general one-sided Jacobi and the select alone.  C128: jacobi_rows_cplx_kernel (force_global is ignored), S stays real"""
    t = {F32: np.float32, F64: np.float64, C128: np.complex128}[dtype]
    M = np.ascontiguousarray(M, dtype=t).copy()
    nb, m, ln = M.shape
    Vt = np.zeros((nb, k, ln), dtype=t)
    S = np.zeros((nb, k), dtype=np.float64 if dtype == C128 else t)
    sw = np.zeros(nb, dtype=np.int32)
    rc = lib().pepsgpu_diag_jacobi(dtype, M.ctypes.data_as(C.c_void_p), m, ln, nb, k, Vt.ctypes.data_as(C.c_void_p),
                                   S.ctypes.data_as(C.c_void_p), int(force_global), _ip(sw))
    if rc != 0:
        raise RuntimeError("diag_jacobi failed: %s" % lib().pepsgpu_last_error(None).decode())
    return M, Vt, S, sw & 0xFF      # high bits: diagnostics (rows above the noise floor at entry)


def diag_chol_solve_rows(S, X, rows, run_flag=None):
    """One Cholesky-QR pass X <- L^-1 X, L L^H = S, as the dense truncation routes launch it: S [nb][64][64] (upper triangle read),
    X [nb][r_max][len] (returned, the input is not written).  float64 arrays: chol_solve_rows_kernel, rows [nb]; complex128:
    chol_solve_rows_cplx_kernel, rows a single int.  run_flag [nb]: entries with run_flag[b] >= 0 are left alone."""
    cplx = np.iscomplexobj(X)
    t = np.complex128 if cplx else np.float64
    S = np.ascontiguousarray(S, dtype=t)
    X = np.ascontiguousarray(X, dtype=t).copy()
    nb, r_max, ln = X.shape
    assert S.shape == (nb, 64, 64)
    if cplx:
        r, rows_a = int(rows), None
    else:
        r, rows_a = 0, np.ascontiguousarray(rows, dtype=np.int32)
        assert rows_a.shape == (nb,)
    flag = None if run_flag is None else np.ascontiguousarray(run_flag, dtype=np.int32)
    rc = lib().pepsgpu_diag_chol_solve_rows(int(cplx), S.ctypes.data_as(C.c_void_p), X.ctypes.data_as(C.c_void_p), nb, r_max, ln,
                                            None if rows_a is None else _ip(rows_a), r, None if flag is None else _ip(flag))
    if rc != 0:
        raise RuntimeError("diag_chol_solve_rows failed: %s" % lib().pepsgpu_last_error(None).decode())
    return X


def diag_gather_rows(M, piv, rows, run_flag=None, fill=0.0):
    """gather_rows_kernel alone: Q[b][j] = M[b][piv[b][j]] for j < rows[b] where piv >= 0.  M [nb][m][len] float64 or complex128,
    piv [nb][slots]; returns Q [nb][64][len], `fill` wherever the kernel stores nothing."""
    cplx = np.iscomplexobj(M)
    t = np.complex128 if cplx else np.float64
    M = np.ascontiguousarray(M, dtype=t)
    nb, m, ln = M.shape
    piv = np.ascontiguousarray(piv, dtype=np.int32)
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    assert piv.ndim == 2 and piv.shape[0] == nb and rows.shape == (nb,)
    flag = None if run_flag is None else np.ascontiguousarray(run_flag, dtype=np.int32)
    Q = np.full((nb, 64, ln), fill, dtype=t)
    rc = lib().pepsgpu_diag_gather_rows(int(cplx), M.ctypes.data_as(C.c_void_p), nb, m, ln, _ip(piv), piv.shape[1], _ip(rows),
                                        None if flag is None else _ip(flag), Q.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise RuntimeError("diag_gather_rows failed: %s" % lib().pepsgpu_last_error(None).decode())
    return Q


def diag_sign_table(rows, cols, complex=False):
    """sign_table_kernel alone: the [rows][cols] table of +1 / -1 the complex range finder starts from"""
    out = np.zeros((rows, cols), dtype=np.complex128 if complex else np.float64)
    rc = lib().pepsgpu_diag_sign_table(int(bool(complex)), rows, cols, out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise RuntimeError("diag_sign_table failed: %s" % lib().pepsgpu_last_error(None).decode())
    return out


def diag_trunc_rows(M, rows, k, span, fill=0.0):
    """The short-row Jacobi with its select epilogue alone (the launch of a low-rank site): M [nb][m][len] float32, rows[b] live
    rows, k rows of Vt per entry, span: ask for the span path.  Returns Vt [nb][k][len], klive [nb] and the sweeps words
    (sweeps | live << 8); entries the kernel does not take (0 or more than 16 live rows) keep `fill` / -1 / -1."""
    M = np.ascontiguousarray(M, dtype=np.float32)
    nb, m, ln = M.shape
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    assert rows.shape == (nb,)
    Vt = np.full((nb, k, ln), fill, dtype=np.float32)
    kl = np.full(nb, -1, dtype=np.int32)
    sw = np.full(nb, -1, dtype=np.int32)
    rc = lib().pepsgpu_diag_trunc_rows(M.ctypes.data_as(C.c_void_p), m, ln, nb, _ip(rows), int(k), int(bool(span)),
                                       Vt.ctypes.data_as(C.c_void_p), _ip(kl), _ip(sw))
    if rc != 0:
        raise RuntimeError("diag_trunc_rows failed: %s" % lib().pepsgpu_last_error(None).decode())
    return Vt, kl, sw


class Walker:
    """BMPSContractor::BMPSWalker (bmps_contractor.h:357-646) for all Monte-Carlo walkers of a context: method names follow the
    reference.  The TransferMPO is set once (set_mpo / set_mpo_states / set_mpo_tensors); `opp_level` names the opposite
    boundary = level of the DOWN stack (down_stack[opp_level] in the reference's tests).
    Lifetime: the device copy is released by destroy(), at the end of a `with ctx.get_walker(...) as w:` block, or when the object is
    collected; Context.set_configs invalidates every walker of the context."""

    def __init__(self, ctx, wid):
        self.ctx, self.wid = ctx, wid

    def _info(self):
        v = np.zeros(4, dtype=np.int32)
        c = self.ctx
        c._ck(c._l.pepsgpu_walker_info(c._h, self.wid, _ip(v[0:1]), _ip(v[1:2]), _ip(v[2:3]), _ip(v[3:4])))
        return v

    def GetPosition(self): return int(self._info()[0])
    def GetStackSize(self): return int(self._info()[1])
    def GetBTenLeftCol(self): return int(self._info()[2])
    def GetBTenRightCol(self): return int(self._info()[3])

    def set_mpo(self, num):
        c = self.ctx
        c._ck(c._l.pepsgpu_walker_set_mpo(c._h, self.wid, num, None, None, 0))

    def set_mpo_states(self, num, states):
        c = self.ctx
        st = np.ascontiguousarray(states, dtype=np.int32)
        assert st.ndim == 2 and st.shape[0] == c.n
        c._ck(c._l.pepsgpu_walker_set_mpo(c._h, self.wid, num, _ip(st), None, 0))

    def set_mpo_tensors(self, num, tensors):
        """tensors [nt][N][D][D][D][D] (leg order L, D, R, U, zero padded to D), nt = 1 or n"""
        c = self.ctx
        t = np.ascontiguousarray(tensors, dtype=c._ot)
        assert t.ndim == 6 and t.shape[2:] == (c.D,) * 4
        c._ck(c._l.pepsgpu_walker_set_mpo(c._h, self.wid, num, None, _dp(t), t.shape[0]))

    def set_mpo_excited(self, num, col, state_map):
        """the MPO becomes row `num` under the walkers' configurations with the state s of site `col` replaced by state_map[s]
        (phys_dim entries), built on the device; returns the open mask [n] (bool): state_map[s] != s"""
        c = self.ctx
        sm = np.ascontiguousarray(state_map, dtype=np.int32)
        assert sm.shape == (c.d,), sm.shape
        op = np.zeros(c.n, dtype=np.uint8)
        c._ck(c._l.pepsgpu_walker_set_mpo_excited(c._h, self.wid, num, col, _ip(sm), op.ctypes.data_as(C.POINTER(C.c_uint8))))
        return op.astype(bool)

    def trace_slice(self, opp_level, site_map, mask=None):
        """InitBTenLeft / InitBTenRight and the right-to-left scan of TraceWithBTen + GrowBTenRightStep over the row of the current
        MPO in one call: [n][cols], entry (w, x) = the trace with the state s of site x replaced by site_map[s] where mask[w]
        (None: every walker) and site_map[s] != s, exactly 0 elsewhere"""
        c = self.ctx
        sm = np.ascontiguousarray(site_map, dtype=np.int32)
        assert sm.shape == (c.d,), sm.shape
        mk = None if mask is None else np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        assert mk is None or mk.shape == (c.n,), mk.shape
        out = np.zeros((c.n, c.cols), dtype=c._ot)
        c._ck(c._l.pepsgpu_walker_trace_slice(c._h, self.wid, opp_level, _ip(sm),
                                              None if mk is None else mk.ctypes.data_as(C.POINTER(C.c_uint8)), _dp(out)))
        return out

    def set_mpo_excited_pair(self, num, col, nf, pair_table, slot=0):
        """the MPO becomes row `num` under the walkers' configurations with the pair (col, col + 1) replaced by candidate `slot` of
        pair_table ([d * d][2][2] over physical states, nf [d] their fermion numbers), built on the device; returns (open [n] bool,
        sign [n] = Sigma(S') / Sigma(S), 0 for none)"""
        c = self.ctx
        occ = np.ascontiguousarray(nf, dtype=np.int32)
        tab = np.ascontiguousarray(pair_table, dtype=np.int32)
        assert tab.size == 4 * occ.size ** 2, tab.shape
        op, sg = np.zeros(c.n, dtype=np.uint8), np.zeros(c.n, dtype=np.int32)
        c._ck(c._l.pepsgpu_walker_set_mpo_excited_pair(c._h, self.wid, num, col, occ.size, _ip(occ), _ip(tab), slot,
                                                       op.ctypes.data_as(C.POINTER(C.c_uint8)), _ip(sg)))
        return op.astype(bool), sg

    def pair_trace_slice(self, opp_level, nf, pair_table, mask=None):
        """InitBTenLeft(0) / InitBTenRight(1) and the left-to-right scan of TraceWithTwoSiteBTen + ShiftBTenWindow(RIGHT) over the row
        of the current MPO in one call: [n][cols - 1][2], entry (w, x, k) = sign * the trace with the states of (x, x + 1) replaced by
        candidate k of pair_table where mask[w] (None: every walker) and the candidate exists, exactly 0 elsewhere"""
        c = self.ctx
        occ = np.ascontiguousarray(nf, dtype=np.int32)
        tab = np.ascontiguousarray(pair_table, dtype=np.int32)
        assert tab.size == 4 * occ.size ** 2, tab.shape
        mk = None if mask is None else np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        assert mk is None or mk.shape == (c.n,), mk.shape
        out = np.zeros((c.n, c.cols - 1, 2), dtype=c._ot)
        c._ck(c._l.pepsgpu_walker_pair_trace_slice(c._h, self.wid, opp_level, occ.size, _ip(occ), _ip(tab),
                                                   None if mk is None else mk.ctypes.data_as(C.POINTER(C.c_uint8)), _dp(out)))
        return out

    def Evolve(self): self.ctx._ck(self.ctx._l.pepsgpu_walker_evolve(self.ctx._h, self.wid))
    def EvolveStep(self): self.ctx._ck(self.ctx._l.pepsgpu_walker_evolve_step(self.ctx._h, self.wid))

    def ContractRow(self, opp_level):
        c = self.ctx
        out = np.zeros(c.n, dtype=c._ot)
        c._ck(c._l.pepsgpu_walker_contract_row(c._h, self.wid, opp_level, _dp(out)))
        return out

    def InitBTenLeft(self, opp_level, target_col): self.ctx._ck(self.ctx._l.pepsgpu_walker_init_bten(self.ctx._h, self.wid, opp_level, LEFT, target_col))
    def InitBTenRight(self, opp_level, target_col): self.ctx._ck(self.ctx._l.pepsgpu_walker_init_bten(self.ctx._h, self.wid, opp_level, RIGHT, target_col))
    def GrowBTenLeftStep(self, opp_level): self.ctx._ck(self.ctx._l.pepsgpu_walker_grow_bten_step(self.ctx._h, self.wid, opp_level, LEFT))
    def GrowBTenRightStep(self, opp_level): self.ctx._ck(self.ctx._l.pepsgpu_walker_grow_bten_step(self.ctx._h, self.wid, opp_level, RIGHT))
    def ShiftBTenWindow(self, opp_level, position): self.ctx._ck(self.ctx._l.pepsgpu_walker_shift_bten_window(self.ctx._h, self.wid, opp_level, position))
    def ClearBTen(self): self.ctx._ck(self.ctx._l.pepsgpu_walker_clear_bten(self.ctx._h, self.wid))

    def _trace(self, opp_level, site_col, two, states, tensors):
        c = self.ctx
        out = np.zeros(c.n, dtype=c._ot)
        st = None if states is None else np.ascontiguousarray(states, dtype=np.int32)
        tt = None if tensors is None else np.ascontiguousarray(tensors, dtype=c._ot)
        nt = 0
        if tt is not None:
            tt = tt.reshape((-1,) + ((2,) if two else ()) + (c.D,) * 4)
            nt = tt.shape[0]
        c._ck(c._l.pepsgpu_walker_trace_with_bten(c._h, self.wid, opp_level, site_col, int(two), None if st is None else _ip(st),
                                                  None if tt is None else _dp(tt), nt, _dp(out)))
        return out

    def TraceWithBTen(self, opp_level, site_col, states=None, tensors=None):
        """states [n] (SITPS component per walker) or tensors [nt][D^4]; neither: the MPO's own tensor"""
        return self._trace(opp_level, site_col, False, states, tensors)

    def TraceWithTwoSiteBTen(self, opp_level, site_col, states=None, tensors=None):
        """states [n][2] or tensors [nt][2][D^4]"""
        return self._trace(opp_level, site_col, True, states, tensors)

    def GetBMPSTensor(self, idx):
        c = self.ctx
        dims = np.zeros(3, dtype=np.int32)
        c._ck(c._l.pepsgpu_walker_get_bmps_tensor(c._h, self.wid, idx, _ip(dims), None, None))
        data = np.zeros((c.n,) + tuple(int(x) for x in dims), dtype=c._ot)
        ls = np.zeros(c.n, dtype=np.float64)
        c._ck(c._l.pepsgpu_walker_get_bmps_tensor(c._h, self.wid, idx, _ip(dims), _dp(data), _dp(ls)))
        return data, ls

    def clone(self):
        """copy construction (`auto excited_walker = main_walker;`)"""
        wid = np.zeros(1, dtype=np.int32)
        self.ctx._ck(self.ctx._l.pepsgpu_walker_clone(self.ctx._h, self.wid, _ip(wid)))
        return Walker(self.ctx, int(wid[0]))

    def destroy(self):
        if self.wid is not None:
            self.ctx._ck(self.ctx._l.pepsgpu_walker_destroy(self.ctx._h, self.wid))
            self.wid = None

    # A walker is a deep copy of one boundary MPS for ALL Monte-Carlo walkers of the context: release it with the object, as the
    # destructor of the C++ BMPSWalker does.  The error code is ignored here -- set_configs / close of the context drop every walker
    # (a stale object then finds "no such walker"), and a context that is already closed has nothing left to free.
    def _release_quietly(self):
        wid, self.wid = self.wid, None
        ctx = self.ctx
        if wid is not None and getattr(ctx, "_h", None):
            try:
                ctx._l.pepsgpu_walker_destroy(ctx._h, wid)
            except Exception:
                pass

    def __del__(self):
        # The documented release paths are destroy() and the context manager.  A finalizer must not enter the engine (it may run on
        # another thread while a call on the same context is in flight: ctypes releases the GIL): it queues the id, the context frees
        # it at its next call from the owning thread (_ReapingLib) or drops it with close().
        try:
            wid, self.wid = self.wid, None
            if wid is not None and getattr(self.ctx, "_h", None):
                q = getattr(self.ctx, "_dead_walkers", None)
                if q is None:
                    q = self.ctx._dead_walkers = []
                q.append(wid)
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self._release_quietly()
        return False
