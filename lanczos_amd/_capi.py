"""ctypes binding of liblanczos_hip.so (include/lanczos_hip.h).

The library is the only compute backend of this package: if it cannot be
loaded, or no GPU is present, every compute call raises - there is no CPU
fallback (the NumPy path is the reference's own and lives, as a checker, under
oracle/ for the tests only).
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblanczos_hip.so")

LZ_OK = 0
LZ_WARN_BREAKDOWN = 1
STATUS_NAMES = {0: "LZ_OK", 1: "LZ_WARN_BREAKDOWN", -1: "LZ_ERR_ARG", -2: "LZ_ERR_HIP", -3: "LZ_ERR_COMM", -4: "LZ_ERR_STATE", -5: "LZ_ERR_NOMEM", -6: "LZ_ERR_NODEVICE"}

FLAG_PROFILE = 1
FLAG_QTW_MFMA = 2
FLAG_QTW_VALU = 4
FLAG_SPMV_SCALAR = 8
FLAG_FUSED_NORM = 16
FLAG_SPMV_STREAM = 32
FLAG_REORTH_PARTIAL = 64
FLAG_OVERLAP_HALO = 128
FLAG_ONE_REDUCE = 256
FLAG_TRL_PASS2_ALWAYS = 512  # thick-restart Lanczos: the second Gram-Schmidt pass at every extension step (default: where DGKS asks for it)
FLAG_TRL_FILTER_UNFUSED = 1024  # thick-restart Lanczos: every Chebyshev filter step as SpMV + recurrence kernel, never the fused SpMV epilogue (A/B, tests)

# lz_set_tuning knob indices (the legend lives in include/lanczos_hip.h)
TUNE_QTW_SLICE = 0          # Q^T w slice length per block
TUNE_QTW_VARIANT = 1        # Q^T w kernel variant (unroll / rows per tile; >= 20: timing-only ablations, kernel-bench build)
TUNE_STREAM_ROWS = 2        # CSR-stream rows per block
TUNE_SPMV_ABLATION = 3      # (removed in round 5: the timing-only SpMV ablation arms; any non-zero value is refused)
TUNE_STREAM_ENTRIES = 4     # CSR-stream entries per block
TUNE_FIXED_ROWS = 5         # fixed-K rows per block (CSR-order kernel)
TUNE_FORCE_COLLECTIVES = 6  # issue the collectives even when world == 1
TUNE_PROFILE_STRIDE = 7     # bracket only every value-th iteration of lz_run with events
TUNE_UPDATE_VARIANT = 8     # pass-2 kernel variant
TUNE_RITZ_KERNEL = 9        # Ritz back-transform kernel (0 auto, 1 the one-workgroup-per-128-rows kernel always)
TUNE_PB_ENTRIES = 10        # two-phase SpMV: entries per row block
TUNE_BI_LINKS = 11          # two-sided Gram-Schmidt links
TUNE_NO_SKEW = 12           # 1 = no row-stride skew
TUNE_POISON_BASIS = 13      # 1 = NaN-poison a fresh basis allocation (test knob)
TUNE_SPMV_PLAN = 14         # irregular SpMV plan (0 auto, 1 never two-phase, 2 always)
TUNE_LOOP = 15              # loop structure (0 auto, 1 six launches per step always, 6 the one-sweep loop at any size (never pairs), 7 the same, never fused,
                            # 8 the one-sweep loop at any size with pair walks, 9 the same with 16 positions per lane in the pair walk,
                            # 10 / 11 with group walks, 4 / 8 positions per lane; 12 groups with the scaled chain, 13 groups without the side stream: A/B)
TUNE_RITZ_CHUNK_ROWS = 16   # rows per chunk of the chunked Ritz mode (> 0 forces it)
TUNE_FIXED_LAYOUT = 17      # fixed-K SpMV layout (0 auto: row-class coded ELL where the rows fall into classes, else CSR order and ELL only in the partial loop;
                            # 1 never ELL; 2 / 3 uncoded ELL always, one / two rows per lane; 4 offsets-only coding)
TUNE_GRAM_KERNEL = 19       # Gram matrix of the Ritz vectors (0 auto: symmetric accumulator-stationary kernel with LDS-staged operands, 1 split-K TN GEMM, 2 the register-ring form)
TUNE_CLS_GROUP = 23         # fully coded SpMV: 0 two adjacent rows per lane; 1 / 3 one row per lane, one / two units per workgroup (A/B)
TUNE_PB_GROUPS = 22         # two-phase SpMV: phases interleaved over this many row-block groups (A/B arm; 0 = off)
TUNE_GRAM_SLICES = 21       # Gram matrix: K slices of the symmetric kernel (0 auto)
TUNE_PARTIAL_LOOKAHEAD = 20 # one-reduce partial loop: safety factor of the look-ahead sweep decision (0 = default 4)
TUNE_PARTIAL_LOOP = 18      # partial re-orthogonalisation loop (0 device-resident, 1 host-decided, 2 device-resident without the fused scale,
                            # 3 device-resident with a separate second-stage kernel behind pass 1)

KERNEL_CLASSES = ("spmv", "qtw", "update", "three_term", "final", "comm", "ritz")
K_COUNT = len(KERNEL_CLASSES)


class LzTimings(C.Structure):
    _fields_ = [
        ("ms", C.c_double * K_COUNT),
        ("timed_bytes", C.c_double * K_COUNT),
        ("timed_launches", C.c_int64 * K_COUNT),
        ("bytes", C.c_double * K_COUNT),
        ("flops", C.c_double * K_COUNT),
        ("launches", C.c_int64 * K_COUNT),
        ("total_ms", C.c_double),
    ]


HOST_ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int64)
HOST_EXCHANGE_FN = C.CFUNCTYPE(
    C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_int64)
)
HOST_ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int64)

_P = C.c_void_p
_D = C.POINTER(C.c_double)
_I32 = C.POINTER(C.c_int32)
_I64 = C.POINTER(C.c_int64)

# name -> (restype, argtypes): every symbol include/lanczos_hip.h declares
SIGNATURES = {
    "lz_version": (C.c_int, []),
    "lz_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "lz_create": (C.c_int, [C.POINTER(_P), C.c_int]),
    "lz_destroy": (C.c_int, [_P]),
    "lz_last_error": (C.c_char_p, [_P]),
    "lz_set_options": (C.c_int, [_P, C.c_int]),
    "lz_set_tuning": (C.c_int, [_P, C.c_int, C.c_int]),
    "lz_runtime_info": (C.c_int, [C.c_char_p, C.c_size_t]),
    "lz_device_synchronize": (C.c_int, [_P]),
    "lz_device_memory": (C.c_int, [_P, _I64, _I64]),
    "lz_device_name": (C.c_int, [_P, C.c_char_p, C.c_size_t]),
    "lz_padded_rows": (C.c_int64, [C.c_int64]),
    "lz_comm_load": (C.c_int, []),
    "lz_comm_unique_id": (C.c_int, [_P, C.c_size_t]),
    "lz_comm_init_rccl": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_size_t]),
    "lz_comm_init_host": (C.c_int, [_P, C.c_int, C.c_int, HOST_ALLREDUCE_FN, HOST_EXCHANGE_FN, HOST_ALLGATHER_FN, _P]),
    "lz_set_csr": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _I32, _I32, _D]),
    "lz_set_dense": (C.c_int, [_P, C.c_int64, _D]),
    "lz_set_dense_block": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _D]),
    "lz_build_stencil3d": (C.c_int, [_P, C.c_int, C.c_int, C.c_double, _D, _D, C.c_int]),
    "lz_build_stencil3d_block": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, _D, C.c_int, _D, C.c_int, C.c_int64, C.c_int64,
                                           C.c_int, _I64, _I64]),
    "lz_csr_info": (C.c_int, [_P, _I64, _I64]),
    "lz_spmv_plan": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "lz_spmv_coding": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "lz_get_csr": (C.c_int, [_P, _I32, _I32, _D]),
    "lz_set_halo": (C.c_int, [_P, C.c_int, _I32, _I64, _I32, _I64]),
    "lz_set_allgather": (C.c_int, [_P, C.c_int64]),
    "lz_reserve": (C.c_int, [_P, C.c_int64, C.c_int, C.c_int]),
    "lz_run": (C.c_int, [_P, C.c_int, _D, _D, _D]),
    "lz_get_residual": (C.c_int, [_P, _D]),
    "lz_run_resume": (C.c_int, [_P, C.c_int, C.c_int, _D, C.c_int64, _D, _D, _D, _D, _D]),
    "lz_get_basis": (C.c_int, [_P, _D, C.c_int64]),
    "lz_get_basis_block": (C.c_int, [_P, C.c_int64, C.c_int64, _D, C.c_int64]),
    "lz_ritz_vectors": (C.c_int, [_P, _D, _D]),
    "lz_get_ritz_vectors": (C.c_int, [_P, _D]),
    "lz_get_ritz_rows": (C.c_int, [_P, C.c_int64, C.c_int64, _D]),
    "lz_ritz_info": (C.c_int, [_P, _I64, _D]),
    "lz_ritz_gram": (C.c_int, [_P, _D]),
    "lz_gram_info": (C.c_int, [_P, _D]),
    "lz_ritz_quality": (C.c_int, [_P, _D]),
    "lz_get_timings": (C.c_int, [_P, C.POINTER(LzTimings)]),
    "lz_last_sweeps": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "lz_last_sweep_misses": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "lz_get_omega_state": (C.c_int, [_P, _D, C.c_int64]),
    "lz_run_resume_partial": (C.c_int, [_P, C.c_int, C.c_int, _D, C.c_int64, _D, _D, _D, _D, _D, _D]),
    "lz_last_sweep_log": (C.c_int, [_P, C.POINTER(C.c_int), C.c_int]),
    "lz_comm_counts": (C.c_int, [_P, _I64, _I64]),
    "lz_last_engine": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "lz_last_gate_trips": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "lz_last_one_sweep_fused": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "lz_last_one_sweep_pairs": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "lz_last_pair_abandoned": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "lz_last_one_sweep_quads": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "lz_last_quad_abandoned": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "lz_one_sweep_host_predict": (C.c_int, [C.c_int, C.c_int, _D, _D, C.c_double, C.c_double, C.c_double, _D]),
    "lz_one_sweep_host_post": (C.c_int, [C.c_int, C.c_int, _D, _D, _D, C.c_double, _D]),
    "lz_last_host_syncs": (C.c_int, [_P, _I64]),
    "lz_basis_alloc": (C.c_int, [_P, C.c_int]),
    "lz_basis_set_row": (C.c_int, [_P, C.c_int, _D]),
    "lz_basis_set_rows": (C.c_int, [_P, C.c_int, C.c_int, _D, C.c_int64]),
    "lz_basis_get_row": (C.c_int, [_P, C.c_int, _D]),
    "lz_r_set": (C.c_int, [_P, _D]),
    "lz_r_get": (C.c_int, [_P, _D]),
    "lz_step_spmv": (C.c_int, [_P, C.c_int, _D]),
    "lz_step_reorth": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _D, _D]),
    "lz_step_three_term": (C.c_int, [_P, C.c_int, C.c_int, C.c_double, C.c_double, _D]),
    "lz_os_state_set": (C.c_int, [_P, C.c_int, _D, _D, _D, C.c_double, C.c_double, C.c_double]),
    "lz_os_step": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "lz_os_state_get": (C.c_int, [_P, C.c_int, C.c_int] + [_D] * 11 + [C.POINTER(C.c_int)] * 3),
    "lz_os_raw_get": (C.c_int, [_P, C.c_int, C.c_int, _D, _D, C.c_int64]),
    "lz_spmv_host": (C.c_int, [_P, _D, _D]),
    "lz_set_csr_transpose": (C.c_int, [_P, C.c_int64, _I32, _I32, _D]),
    "lz_run_two_sided": (C.c_int, [_P, C.c_int, _D, _D, _D, _D, _D]),
    "lz_bi_alloc": (C.c_int, [_P, C.c_int]),
    "lz_bi_set_row": (C.c_int, [_P, C.c_int, C.c_int, _D]),
    "lz_bi_get_row": (C.c_int, [_P, C.c_int, C.c_int, _D]),
    "lz_step_bireorth": (C.c_int, [_P, C.c_int]),
    "lz_step_bireorth_mem_safe": (C.c_int, [_P, C.c_int]),
    "lz_trl_begin": (C.c_int, [_P, C.c_int, _D]),
    "lz_trl_extend": (C.c_int, [_P, C.c_int, C.c_int, _D, _D]),
    "lz_trl_begin_band": (C.c_int, [_P, C.c_int, C.c_int, _D]),
    "lz_trl_extend_band": (C.c_int, [_P, C.c_int, C.c_int, _D, _D]),
    "lz_trl_restart": (C.c_int, [_P, C.c_int, C.c_int, _D]),
    "lz_trl_probe": (C.c_int, [_P, C.c_int, _D]),
    "lz_trl_get_vectors": (C.c_int, [_P, C.c_int, _D]),
    "lz_trl_residuals": (C.c_int, [_P, C.c_int, _D, _D]),
    "lz_trl_residuals_cplx": (C.c_int, [_P, C.c_int, _D, _D, _D]),
    "lz_trl_set_filter": (C.c_int, [_P, C.c_int, _D, _D, C.c_double]),
    "lz_trl_set_series": (C.c_int, [_P, C.c_int, _D, C.c_double, C.c_double]),
    "lz_trl_filter_apply": (C.c_int, [_P, _D, _D]),
    "lz_trl_rayleigh": (C.c_int, [_P, C.c_int, _D]),
    "lz_trl_set_rows": (C.c_int, [_P, C.c_int, C.c_int, _D, C.c_int64]),
    "lz_trl_get_rows": (C.c_int, [_P, C.c_int, C.c_int, _D, C.c_int64]),
    "lz_set_csr_cplx": (C.c_int, [_P, C.c_int64, C.c_int64, _I32, _I32, _D]),
    "lz_set_dense_cplx": (C.c_int, [_P, C.c_int64, _D]),
    "lz_zspmv_host": (C.c_int, [_P, _D, _D]),
    "lz_ztrl_begin": (C.c_int, [_P, C.c_int, _D]),
    "lz_ztrl_extend": (C.c_int, [_P, C.c_int, C.c_int, _D, _D]),
    "lz_ztrl_restart": (C.c_int, [_P, C.c_int, C.c_int, _D]),
    "lz_ztrl_probe": (C.c_int, [_P, C.c_int, _D]),
    "lz_ztrl_get_vectors": (C.c_int, [_P, C.c_int, _D]),
    "lz_ztrl_residuals": (C.c_int, [_P, C.c_int, _D, _D]),
    "lz_ztrl_set_rows": (C.c_int, [_P, C.c_int, C.c_int, _D, C.c_int64]),
    "lz_ztrl_get_rows": (C.c_int, [_P, C.c_int, C.c_int, _D, C.c_int64]),
    "lz_expm_begin": (C.c_int, [_P, C.c_int, C.c_int, _D]),
    "lz_expm_extend": (C.c_int, [_P, C.c_int, C.c_int, _D, _D]),
    "lz_expm_combine": (C.c_int, [_P, C.c_int, C.c_int, _D, _D]),
    "lz_expm_get_rows": (C.c_int, [_P, C.c_int, C.c_int, _D, C.c_int64]),
    "lz_zspmv_real_host": (C.c_int, [_P, _D, _D]),
    "lz_expm_info": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "lz_expm_product_time": (C.c_int, [_P, C.c_int, _D]),
    "lz_expm_set_product": (C.c_int, [_P, C.c_int]),
    "lz_minres_begin": (C.c_int, [_P, _D, _D, C.c_double]),
    "lz_minres_run": (C.c_int, [_P, C.c_int, C.c_double, _D]),
    "lz_minres_history": (C.c_int, [_P, _D, C.c_int]),
    "lz_minres_get": (C.c_int, [_P, C.c_int, _D]),
    "lz_minres_set_state": (C.c_int, [_P, C.c_int, _D, _D, _D, _D, _D, _D]),
    "lz_minres_info": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "lz_minres_step_time": (C.c_int, [_P, C.c_int, _D]),
    "lz_bicgstab_begin": (C.c_int, [_P, _D, _D]),
    "lz_bicgstab_run": (C.c_int, [_P, C.c_int, C.c_double, _D]),
    "lz_bicgstab_history": (C.c_int, [_P, _D, C.c_int]),
    "lz_bicgstab_get": (C.c_int, [_P, C.c_int, _D]),
    "lz_bicgstab_set_state": (C.c_int, [_P, C.c_int, _D, _D, _D, _D, _D, _D]),
    "lz_bicgstab_info": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "lz_bicgstab_step_time": (C.c_int, [_P, C.c_int, _D]),
    "lz_cg_begin": (C.c_int, [_P, _D, _D, _D]),
    "lz_cg_run": (C.c_int, [_P, C.c_int, C.c_double, _D]),
    "lz_cg_history": (C.c_int, [_P, _D, C.c_int]),
    "lz_cg_get": (C.c_int, [_P, C.c_int, _D]),
    "lz_cg_set_state": (C.c_int, [_P, C.c_int, _D, _D, _D, _D, _D]),
    "lz_cg_info": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "lz_cg_step_time": (C.c_int, [_P, C.c_int, _D]),
    "lz_gmres_begin": (C.c_int, [_P, C.c_int, _D, _D]),
    "lz_gmres_run": (C.c_int, [_P, C.c_int, C.c_double, _D]),
    "lz_gmres_end_cycle": (C.c_int, [_P, C.c_double, _D]),
    "lz_gmres_history": (C.c_int, [_P, _D, C.c_int, _D, C.c_int]),
    "lz_gmres_get": (C.c_int, [_P, C.c_int, _D]),
    "lz_gmres_set_state": (C.c_int, [_P, C.c_int, _D, _D, _D, _D, C.c_int, _D]),
    "lz_gmres_step_time": (C.c_int, [_P, C.c_int, _D]),
    "lz_gmres_info": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "lz_lsmr_begin": (C.c_int, [_P, C.c_int, _D, _D, C.c_double]),
    "lz_lsmr_run": (C.c_int, [_P, C.c_int, C.c_double, C.c_double, C.c_double, _D]),
    "lz_lsmr_get": (C.c_int, [_P, C.c_int, _D]),
    "lz_lsmr_set_state": (C.c_int, [_P, C.c_int, C.c_int, _D, _D, _D, _D, _D, _D]),
    "lz_lsmr_history": (C.c_int, [_P, _D, C.c_int]),
    "lz_lsmr_info": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "lz_lsmr_step_time": (C.c_int, [_P, C.c_int, _D]),
    "lz_gk_set_csr": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, _I32, _I32, _D, _I32, _I32, _D]),
    "lz_gk_set_dense": (C.c_int, [_P, C.c_int64, C.c_int64, _D, C.c_int64, C.c_int]),
    "lz_gk_plan": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "lz_gk_begin": (C.c_int, [_P, C.c_int, _D]),
    "lz_gk_extend": (C.c_int, [_P, C.c_int, C.c_int, _D, _D, _D]),
    "lz_gk_restart": (C.c_int, [_P, C.c_int, C.c_int, _D, _D]),
    "lz_gk_probe": (C.c_int, [_P, C.c_int, C.c_int, _D]),
    "lz_gk_get_vectors": (C.c_int, [_P, C.c_int, C.c_int, _D]),
    "lz_gk_set_rows": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _D, C.c_int64]),
    "lz_gk_get_rows": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _D, C.c_int64]),
    "lz_gk_residuals": (C.c_int, [_P, C.c_int, _D, _D]),
    "lz_gk_spmv": (C.c_int, [_P, C.c_int, _D, _D]),
    "lz_gk_spmv_time": (C.c_int, [_P, C.c_int, C.c_int, _D]),
}


class LanczosHipError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {message}")
        self.status = status


KBENCH_LIB_PATH = os.path.join(_HERE, "liblanczos_kbench.so")  # kernel-bench build: retired A/B arms + timing-only ablations (tools/, tests of those arms)

_lib = None
_live_handles = None  # weakref.WeakSet of open Handle objects, closed by an atexit hook (see Handle)


def mapped_runtimes():
    """{"amdhip64": [paths], "hsa-runtime64": [...], "rccl": [...]} of the ROCm runtime copies mapped into THIS process
    (from /proc/self/maps).  More than one libamdhip64 means two HIP runtimes share the process - what happens when
    PyTorch (which bundles its own ROCm libraries under torch/lib, found through unversioned NEEDED names that never
    match the system sonames) is imported AFTER this library was loaded; DESIGN.md section 5 has the round-1 abort it caused."""
    import re

    found = {"amdhip64": set(), "hsa-runtime64": set(), "rccl": set()}
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                m = re.search(r"(/\S*lib(amdhip64|hsa-runtime64|rccl)\.so\S*)", line)
                if m:
                    found[m.group(2)].add(m.group(1))
    except OSError:
        pass
    return {k: sorted(v) for k, v in found.items()}


def check_single_runtime():
    """Raise if two HIP runtimes are mapped (see ``mapped_runtimes``)."""
    hip = mapped_runtimes()["amdhip64"]
    if len(hip) > 1:
        raise LanczosHipError(-4, "two HIP runtimes are mapped into this process (" + ", ".join(hip) + "): torch must be imported BEFORE "
                              "lanczos_amd.load_library() so that liblanczos_hip.so binds to the runtime torch brings, "
                              "or keep torch out of the process (SocketBootstrap needs none)")


def load_library(path=None):
    """dlopen the HIP extension and bind every declared symbol.  Raises
    ``LanczosHipError`` (never falls back) when the library is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    # The host driver of this pool only supports dmabuf IPC: without this RCCL's cross-process buffer sharing fails with
    # "hipIpcGetMemHandle: invalid argument".  Must be in the environment before the HIP runtime initialises.
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if not os.path.isfile(p):
        raise LanczosHipError(-6, f"HIP extension not built: {p} is missing (run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C lanczos_amd/csrc`)")
    try:
        # default (RTLD_LOCAL) scope: nothing in this library is meant to interpose on, or be interposed by, another
        # ROCm copy in the process
        lib = C.CDLL(p)
    except OSError as e:  # missing libamdhip64 etc.
        raise LanczosHipError(-6, f"cannot load {p}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def runtime_info():
    """{"hip": path of the libamdhip64 the library is bound to, "rccl": path of the librccl it opened ('' if none yet)}."""
    buf = C.create_string_buffer(1024)
    load_library().lz_runtime_info(buf, 1024)
    return dict(kv.split("=", 1) for kv in buf.value.decode().split(";"))


def _close_live_handles():
    # Runs from atexit, i.e. BEFORE the interpreter tears modules down and long before the HIP runtime's own exit
    # handlers / static destructors: device memory, streams and the RCCL communicator are released while the runtime
    # that owns them is still alive (Handle.__del__ at interpreter shutdown may run after it is gone).
    if _live_handles is not None:
        for h in list(_live_handles):
            try:
                h.close()
            except Exception:
                pass


def preload_rccl():
    """dlopen the system RCCL now (before any other library maps a different copy of librccl.so.1)."""
    lib = load_library()
    st = lib.lz_comm_load()
    if st != LZ_OK:
        raise LanczosHipError(st, lib.lz_last_error(None).decode())


def dptr(a):
    return a.ctypes.data_as(_D)


def i32ptr(a):
    return a.ctypes.data_as(_I32)


def i64ptr(a):
    return a.ctypes.data_as(_I64)


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def c128(a):
    """C-contiguous complex128: NumPy's interleaved (re, im) doubles, which is what the ``lz_*_cplx`` / ``lz_z*`` calls take"""
    return np.ascontiguousarray(a, dtype=np.complex128)


class Handle:
    """Thin RAII wrapper over ``lz_handle``: raises on every non-zero status."""

    def __init__(self, device_id=0, lib=None):
        """``lib``: another build of the library (``load_library(KBENCH_LIB_PATH)``: the kernel-bench build); default the product."""
        self.lib = lib if lib is not None else load_library()
        self.matrix_uploads = 0  # lz_set_csr / lz_set_dense / stencil assemblies issued through this handle
        self._h = _P()
        st = self.lib.lz_create(C.byref(self._h), int(device_id))
        if st != LZ_OK:
            msg = self.lib.lz_last_error(None).decode()
            self._h = None
            raise LanczosHipError(st, msg)
        self._keep = []  # keeps ctypes callbacks alive
        self._reserve_lock = threading.Lock()  # lz_reserve may run on a helper thread: it must not meet lz_destroy
        self.breakdown = False
        global _live_handles
        if _live_handles is None:
            import atexit
            import weakref

            _live_handles = weakref.WeakSet()
            atexit.register(_close_live_handles)
        _live_handles.add(self)

    def check(self, st):
        if st != LZ_OK:
            raise LanczosHipError(st, self.lib.lz_last_error(self._h).decode())

    def close(self):
        lock = getattr(self, "_reserve_lock", None)
        if lock is not None:
            lock.acquire()
        try:
            if getattr(self, "_h", None):
                self.lib.lz_destroy(self._h)
                self._h = None
        finally:
            if lock is not None:
                lock.release()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- info / options
    def device_name(self):
        buf = C.create_string_buffer(256)
        self.check(self.lib.lz_device_name(self._h, buf, 256))
        return buf.value.decode()

    def set_options(self, flags):
        self.check(self.lib.lz_set_options(self._h, int(flags)))

    def set_tuning(self, index, value):
        self.check(self.lib.lz_set_tuning(self._h, int(index), int(value)))

    def synchronize(self):
        self.check(self.lib.lz_device_synchronize(self._h))

    def padded_rows(self, rows):
        return int(self.lib.lz_padded_rows(int(rows)))

    # -- communication
    def unique_id(self):
        buf = C.create_string_buffer(128)
        st = self.lib.lz_comm_unique_id(buf, 128)
        if st != LZ_OK:
            raise LanczosHipError(st, self.lib.lz_last_error(None).decode())
        return buf.raw

    def comm_init_rccl(self, world, rank, uid):
        buf = C.create_string_buffer(bytes(uid), 128)
        self.check(self.lib.lz_comm_init_rccl(self._h, int(world), int(rank), buf, 128))

    def comm_init_host(self, world, rank, allreduce, exchange=None, allgather=None):
        """``allreduce(np.ndarray)`` sums in place over ranks; ``exchange(peers, send_segments) -> recv_segments``;
        ``allgather(np.ndarray) -> np.ndarray (world*count)``."""

        def _ar(user, buf, count):
            try:
                a = np.ctypeslib.as_array(buf, shape=(count,))
                allreduce(a)
                return 0
            except Exception:  # pragma: no cover - surfaced as LZ_ERR_COMM
                import traceback

                traceback.print_exc()
                return 1

        def _ex(user, npeers, peers, sendbuf, scount, recvbuf, rcount):
            try:
                pr = [int(peers[i]) for i in range(npeers)]
                sc = [int(scount[i]) for i in range(npeers)]
                rc = [int(rcount[i]) for i in range(npeers)]
                s = np.ctypeslib.as_array(sendbuf, shape=(max(sum(sc), 1),))
                r = np.ctypeslib.as_array(recvbuf, shape=(max(sum(rc), 1),))
                so = np.concatenate([[0], np.cumsum(sc)]).astype(int)
                ro = np.concatenate([[0], np.cumsum(rc)]).astype(int)
                out = exchange(pr, [s[so[i] : so[i + 1]].copy() for i in range(npeers)], rc)
                for i in range(npeers):
                    r[ro[i] : ro[i + 1]] = out[i]
                return 0
            except Exception:  # pragma: no cover
                import traceback

                traceback.print_exc()
                return 1

        def _ag(user, sendbuf, recvbuf, count):
            try:
                s = np.ctypeslib.as_array(sendbuf, shape=(count,))
                r = np.ctypeslib.as_array(recvbuf, shape=(count * world,))
                r[:] = allgather(s.copy())
                return 0
            except Exception:  # pragma: no cover
                import traceback

                traceback.print_exc()
                return 1

        cbs = (HOST_ALLREDUCE_FN(_ar), HOST_EXCHANGE_FN(_ex), HOST_ALLGATHER_FN(_ag))
        self._keep.append(cbs)
        self.check(self.lib.lz_comm_init_host(self._h, int(world), int(rank), cbs[0], cbs[1], cbs[2], None))

    # -- matrix
    def set_csr(self, M_global, row0, rowptr, colidx, vals, ncols_ext=None):
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
        colidx = np.ascontiguousarray(colidx, dtype=np.int32)
        vals = f64(vals)
        rows = len(rowptr) - 1
        nnz = int(rowptr[-1])
        if ncols_ext is None:
            ncols_ext = M_global
        self.check(self.lib.lz_set_csr(self._h, int(M_global), int(row0), rows, int(ncols_ext), nnz, i32ptr(rowptr), i32ptr(colidx), dptr(vals)))
        self.rows = rows
        self.matrix_uploads += 1

    def set_dense(self, A):
        A = f64(A)
        if A.ndim != 2 or A.shape[0] != A.shape[1]:
            raise ValueError("dense H must be square")
        self.check(self.lib.lz_set_dense(self._h, A.shape[0], dptr(A)))
        self.rows = A.shape[0]
        self.matrix_uploads += 1

    def set_dense_block(self, M_global, row0, A_block):
        """Row block of a dense matrix split over ranks; columns already in the all-gather layout (see the header)."""
        A_block = f64(A_block)
        rows, ncols_ext = A_block.shape
        self.check(self.lib.lz_set_dense_block(self._h, int(M_global), int(row0), rows, ncols_ext, dptr(A_block)))
        self.rows = rows
        self.matrix_uploads += 1

    def build_stencil3d(self, N, points, T_factor, weights4, potential=None, negate_T=False):
        w = f64(weights4)
        assert w.shape == (4,)
        pot = None if potential is None else f64(potential).reshape(-1)
        if pot is not None and pot.shape != (N**3,):
            raise ValueError("potential must have N^3 entries")
        self.check(self.lib.lz_build_stencil3d(self._h, int(N), int(points), float(T_factor), dptr(w), None if pot is None else dptr(pot), int(bool(negate_T))))
        self.rows = N**3

    def build_stencil3d_block(self, dims, points, T_factor, weights4, row0, rows_local, ghost_ranges=(), potential=None,
                              potential_params=None, negate_T=False):
        """Row block ``[row0, row0 + rows_local)`` of the periodic ``Nx x Ny x Nz`` stencil operator, assembled on the device.
        ``ghost_ranges``: ``[(global_start, length), ...]`` in ghost-tail order (``partition.plan_stencil_slab``).
        ``potential``: this rank's diagonal (host array) or ``potential_params`` = the 8 device-potential parameters."""
        Nx, Ny, Nz = (int(d) for d in dims)
        w = f64(weights4)
        assert w.shape == (4,)
        kind, pot = 0, None
        if potential_params is not None:
            kind, pot = 2, f64(potential_params)
            assert pot.shape == (8,)
        elif potential is not None:
            kind, pot = 1, f64(potential).reshape(-1)
            if pot.shape != (rows_local,):
                raise ValueError("potential must have one entry per local row")
        gs = np.ascontiguousarray([g[0] for g in ghost_ranges], dtype=np.int64)
        gl = np.ascontiguousarray([g[1] for g in ghost_ranges], dtype=np.int64)
        self.check(self.lib.lz_build_stencil3d_block(self._h, Nx, Ny, Nz, int(points), float(T_factor), dptr(w), kind,
                                                     None if pot is None else dptr(pot), int(bool(negate_T)), int(row0), int(rows_local),
                                                     len(gs), i64ptr(gs) if len(gs) else None, i64ptr(gl) if len(gl) else None))
        self.rows = int(rows_local)
        self.matrix_uploads += 1

    SPMV_PLANS = ("scalar", "csr-stream", "fixed-k", "two-phase", "dense")

    def spmv_plan(self):
        k = C.c_int()
        self.check(self.lib.lz_spmv_plan(self._h, C.byref(k)))
        return self.SPMV_PLANS[k.value]

    SPMV_CODINGS = ("none", "offsets", "offsets+values", "offsets+values, diagonal streamed")

    def spmv_coding(self):
        """row-class coding of a stencil matrix: ("none" | "offsets" | "offsets+values", number of classes)"""
        c, k = C.c_int(), C.c_int()
        self.check(self.lib.lz_spmv_coding(self._h, C.byref(c), C.byref(k)))
        return self.SPMV_CODINGS[c.value], k.value

    def get_csr(self):
        rows, nnz = C.c_int64(), C.c_int64()
        self.check(self.lib.lz_csr_info(self._h, C.byref(rows), C.byref(nnz)))
        rowptr = np.empty(rows.value + 1, dtype=np.int32)
        colidx = np.empty(nnz.value, dtype=np.int32)
        vals = np.empty(nnz.value)
        self.check(self.lib.lz_get_csr(self._h, i32ptr(rowptr), i32ptr(colidx), dptr(vals)))
        return rowptr, colidx, vals

    def set_halo(self, peers, send_counts, send_idx, recv_counts):
        peers = np.ascontiguousarray(peers, dtype=np.int32)
        sc = np.ascontiguousarray(send_counts, dtype=np.int64)
        rc = np.ascontiguousarray(recv_counts, dtype=np.int64)
        si = np.ascontiguousarray(send_idx, dtype=np.int32)
        self.check(self.lib.lz_set_halo(self._h, len(peers), i32ptr(peers), i64ptr(sc), i32ptr(si), i64ptr(rc)))

    def set_allgather(self, chunk):
        self.check(self.lib.lz_set_allgather(self._h, int(chunk)))

    # -- run
    def reserve(self, rows_local, n, with_ritz=True):
        """allocate the basis (and the Ritz vectors) of the coming run now; safe to call from a helper thread (see lz_reserve).
        ``with_ritz``: False the basis only, True both, 2 the Ritz vectors only."""
        with self._reserve_lock:
            if self._h:
                self.check(self.lib.lz_reserve(self._h, int(rows_local), int(n), 2 if with_ritz == 2 else (1 if with_ritz else 0)))

    def run(self, n, v0_local):
        v0 = f64(v0_local)
        if v0.shape != (self.rows,):
            raise ValueError("v0 has the wrong length")
        alpha = np.zeros(n)
        beta = np.zeros(max(n - 1, 1))
        st = self.lib.lz_run(self._h, int(n), dptr(v0), dptr(alpha), dptr(beta))
        self.breakdown = st == LZ_WARN_BREAKDOWN  # positive status: the run completed, coefficients as the reference's (inf/NaN)
        if not self.breakdown:
            self.check(st)
        self.n = n
        return alpha, beta[: n - 1]

    def get_residual(self):
        """r entering step n of the last run (this rank's rows): with the basis and alpha / beta, a checkpoint"""
        r = np.empty(self.rows)
        self.check(self.lib.lz_get_residual(self._h, dptr(r)))
        return r

    def get_omega_state(self):
        """the omega-recurrence state the device-decided partial loop (engine 7) left behind: part of its checkpoint"""
        n = int(self.n)
        out = np.empty(2 + (n + 2) + 3 * (n + 1))
        self.check(self.lib.lz_get_omega_state(self._h, dptr(out), out.size))
        return out

    def run_resume(self, n, V_rows, r, alpha, beta, omega_state=None):
        """continue a run of j0 = len(V_rows) completed steps to n steps in total; returns the full alpha (n), beta (n - 1).
        ``omega_state`` (from ``get_omega_state`` of the j0-step run): continue the device-decided partial loop."""
        V_rows, r, alpha, beta = f64(V_rows), f64(r), f64(alpha), f64(beta)
        j0 = V_rows.shape[0]
        if V_rows.shape != (j0, self.rows) or r.shape != (self.rows,) or alpha.shape != (j0,) or beta.shape != (max(j0 - 1, 0),):
            raise ValueError("checkpoint arrays have the wrong shapes")
        a_out, b_out = np.zeros(n), np.zeros(max(n - 1, 1))
        if beta.size == 0:
            beta = np.zeros(1)
        if omega_state is not None:
            om = f64(omega_state)
            if om.shape != (2 + (j0 + 2) + 3 * (j0 + 1),):
                raise ValueError("omega_state does not belong to a run of %d steps" % j0)
            st = self.lib.lz_run_resume_partial(self._h, int(n), int(j0), dptr(V_rows), self.rows, dptr(r), dptr(alpha), dptr(beta), dptr(om), dptr(a_out),
                                                dptr(b_out))
        else:
            st = self.lib.lz_run_resume(self._h, int(n), int(j0), dptr(V_rows), self.rows, dptr(r), dptr(alpha), dptr(beta), dptr(a_out), dptr(b_out))
        self.breakdown = st == LZ_WARN_BREAKDOWN
        if not self.breakdown:
            self.check(st)
        self.n = n
        return a_out, b_out[: n - 1]

    def get_basis(self):
        V = np.empty((self.n, self.rows))
        self.check(self.lib.lz_get_basis(self._h, dptr(V), self.rows))
        return V

    def get_basis_block(self, r0, r1):
        """(n, r1 - r0): the entries [r0, r1) of every basis vector"""
        r0, r1 = int(r0), int(r1)
        V = np.empty((self.n, r1 - r0))
        self.check(self.lib.lz_get_basis_block(self._h, r0, r1 - r0, dptr(V), r1 - r0))
        return V

    def ritz_vectors(self, S, fetch=True):
        S = f64(S)
        Y = np.empty((self.rows, self.n)) if fetch else None
        self.check(self.lib.lz_ritz_vectors(self._h, dptr(S), dptr(Y) if fetch else None))
        return Y

    def ritz_fetch(self):
        Y = np.empty((self.rows, self.n))
        self.check(self.lib.lz_get_ritz_vectors(self._h, dptr(Y)))
        return Y

    def ritz_fetch_rows(self, r0, r1):
        """rows [r0, r1) of the Ritz vectors, (r1 - r0, n): served from the resident Y or re-formed from the basis (chunked mode)"""
        r0, r1 = int(r0), int(r1)
        Y = np.empty((r1 - r0, self.n))
        self.check(self.lib.lz_get_ritz_rows(self._h, r0, r1 - r0, dptr(Y)))
        return Y

    def ritz_info(self):
        """{"chunk_rows": 0 (Y resident) or the rows per chunk of the chunked mode, "clock_mhz", "cycles_per_tile",
        "mfma_floor_cycles_per_tile", "tiles"}: the last four from the S-stationary kernel's own clock record (0 if another kernel ran)"""
        ch = C.c_int64()
        clk = np.zeros(4)
        self.check(self.lib.lz_ritz_info(self._h, C.byref(ch), dptr(clk)))
        return {"chunk_rows": int(ch.value), "clock_mhz": float(clk[0]), "cycles_per_tile": float(clk[1]), "mfma_floor_cycles_per_tile": float(clk[2]),
                "tiles": int(clk[3])}

    def ritz_gram(self):
        G = np.empty((self.n, self.n))
        self.check(self.lib.lz_ritz_gram(self._h, dptr(G)))
        return G

    def gram_info(self):
        """in-kernel clock record of the last ritz_gram (symmetric kernel only): held clock, cycles per k-step, MFMA issue floor"""
        c = (C.c_double * 4)()
        self.check(self.lib.lz_gram_info(self._h, c))
        return {"shader_clock_mhz": c[0], "cycles_per_kstep": c[1], "mfma_issue_floor_cycles_per_kstep": c[2], "ksteps": int(c[3])}

    def ritz_quality(self):
        q = np.empty(self.n)
        self.check(self.lib.lz_ritz_quality(self._h, dptr(q)))
        return q

    def last_sweeps(self):
        k = C.c_int()
        self.check(self.lib.lz_last_sweeps(self._h, C.byref(k)))
        return k.value

    def device_memory(self):
        """(free, total) bytes of the handle's GPU"""
        f, t = C.c_int64(), C.c_int64()
        self.check(self.lib.lz_device_memory(self._h, C.byref(f), C.byref(t)))
        return f.value, t.value

    def last_sweep_log(self, n=None):
        """per step of the last run: True where the re-orthogonalisation sweep ran (the device's own record for the partial loops)"""
        n = int(self.n if n is None else n)
        buf = (C.c_int * n)()
        self.check(self.lib.lz_last_sweep_log(self._h, buf, n))
        return np.array(buf[:], dtype=bool)

    def last_sweep_misses(self):
        """one-reduce partial loop: vectors the look-ahead gate should have swept and did not (swept one step late)"""
        k = C.c_int()
        self.check(self.lib.lz_last_sweep_misses(self._h, C.byref(k)))
        return k.value

    def last_engine(self):
        """"kernels": six launches per step; "fused": the three-launch path of small problems (second-stage reductions
        and the three-term recurrence folded into their consumer kernels); "three-term-fused": five launches per step (the
        three-term recurrence folded into pass 1; the default between the small problems and 4e6 rows per rank);
        "one-reduce": LZ_FLAG_ONE_REDUCE; "one-reduce-repeated": such a run whose cancellation guard fired and that was
        repeated on the default loop; "partial-device": LZ_FLAG_REORTH_PARTIAL with the omega-recurrence and the sweep decision on
        the device (no host synchronisation inside the run); "partial-one-reduce": the same with ONE all-reduce per step
        (LZ_FLAG_REORTH_PARTIAL | LZ_FLAG_ONE_REDUCE, look-ahead sweep decision); "one-sweep": one walk over the basis per step,
        coefficients predicted from V^T V and checked in the same walk (the default above 4e6 rows on one rank); "step" / "small": the
        retired one-launch-per-step / one-kernel engines (kernel-bench build)."""
        k = C.c_int()
        self.check(self.lib.lz_last_engine(self._h, C.byref(k)))
        return ("kernels", "small", "fused", "three-term-fused", "step", "one-reduce-repeated", "one-reduce", "partial-device", "partial-one-reduce",
                "one-sweep")[k.value]

    def last_gate_trips(self):
        """one-sweep loop: steps of the last run whose predicted coefficients missed by more than the gate (they ran a correcting sweep)"""
        k = C.c_int()
        self.check(self.lib.lz_last_gate_trips(self._h, C.byref(k)))
        return k.value

    def last_one_sweep_fused(self):
        """one-sweep loop: 1 when the last run took the fused form (no three-term pass; the SpMV divides by beta on read), else 0"""
        k = C.c_int()
        self.check(self.lib.lz_last_one_sweep_fused(self._h, C.byref(k)))
        return k.value

    def last_one_sweep_pairs(self):
        """one-sweep loop: pair walks (one walk over the basis per two steps) behind the last run's result; 0 after a run that abandoned them"""
        k = C.c_int()
        self.check(self.lib.lz_last_one_sweep_pairs(self._h, C.byref(k)))
        return k.value

    def last_pair_abandoned(self):
        """one-sweep loop: 1 when the last run tried the pair form, a prediction missed the gate and the run was repeated on the single form"""
        k = C.c_int()
        self.check(self.lib.lz_last_pair_abandoned(self._h, C.byref(k)))
        return k.value

    def last_one_sweep_quads(self):
        """one-sweep loop: group walks (one walk over the basis per four steps) behind the last run's result; 0 after a run that abandoned them"""
        k = C.c_int()
        self.check(self.lib.lz_last_one_sweep_quads(self._h, C.byref(k)))
        return k.value

    def last_quad_abandoned(self):
        """one-sweep loop: 1 when the last run tried the group form, a prediction missed the gate and the run was repeated on the pair form"""
        k = C.c_int()
        self.check(self.lib.lz_last_quad_abandoned(self._h, C.byref(k)))
        return k.value

    def last_host_syncs(self):
        """host <-> device synchronisations inside the last lz_run (between its first and its last launch)"""
        k = C.c_int64()
        self.check(self.lib.lz_last_host_syncs(self._h, C.byref(k)))
        return k.value

    def timings(self):
        t = LzTimings()
        self.check(self.lib.lz_get_timings(self._h, C.byref(t)))
        out = {"total_ms": t.total_ms}
        ar, ex = C.c_int64(), C.c_int64()
        self.check(self.lib.lz_comm_counts(self._h, C.byref(ar), C.byref(ex)))
        out["allreduces"], out["exchanges"] = ar.value, ex.value  # the collectives of this interval by kind
        for i, k in enumerate(KERNEL_CLASSES):
            out[k] = {"ms": t.ms[i], "timed_bytes": t.timed_bytes[i], "timed_launches": int(t.timed_launches[i]),
                      "bytes": t.bytes[i], "flops": t.flops[i], "launches": int(t.launches[i])}
        return out

    # -- single steps
    def basis_alloc(self, n):
        self.check(self.lib.lz_basis_alloc(self._h, int(n)))
        self.n = n

    def basis_set_row(self, j, row):
        row = f64(row)
        assert row.shape == (self.rows,)
        self.check(self.lib.lz_basis_set_row(self._h, int(j), dptr(row)))

    def basis_set_rows(self, j0, rows):
        """rows j0 .. j0 + len(rows) - 1 of the basis from a C-ordered (count, rows_local) array, in one strided copy"""
        rows = f64(rows)
        assert rows.ndim == 2 and rows.shape[1] == self.rows
        self.check(self.lib.lz_basis_set_rows(self._h, int(j0), int(rows.shape[0]), dptr(rows), int(rows.shape[1])))

    def basis_get_row(self, j):
        out = np.empty(self.rows)
        self.check(self.lib.lz_basis_get_row(self._h, int(j), dptr(out)))
        return out

    def r_set(self, r):
        r = f64(r)
        assert r.shape == (self.rows,)
        self.check(self.lib.lz_r_set(self._h, dptr(r)))

    def r_get(self):
        out = np.empty(self.rows)
        self.check(self.lib.lz_r_get(self._h, dptr(out)))
        return out

    def step_spmv(self, j):
        d = C.c_double()
        self.check(self.lib.lz_step_spmv(self._h, int(j), C.byref(d)))
        return d.value

    def step_reorth(self, j, nrows, scale=False):
        beta = C.c_double()
        c = np.empty(nrows)
        self.check(self.lib.lz_step_reorth(self._h, int(j), int(nrows), int(bool(scale)), C.byref(beta), dptr(c)))
        return (beta.value if scale else None), c

    def step_three_term(self, j, jm1, alpha, beta):
        d = C.c_double()
        self.check(self.lib.lz_step_three_term(self._h, int(j), int(jm1), float(alpha), float(beta), C.byref(d)))
        return d.value

    # -- one loop body of the one-sweep loop on a state set from the host (after basis_alloc, basis_set_rows, step_spmv(j - 1))
    def os_state_set(self, j, G, H, chat, alpha_prev, beta_prev, beta_prev2=0.0):
        """``G``, ``H``: ``(n, n)`` arrays indexed ``[row, column]``; ``chat``: the ``j`` un-normalised predictions ``V_i . w_j``"""
        n = self.n
        Gd, Hd = f64(np.asarray(G).T), f64(np.asarray(H).T)  # the device keeps column i at [i * n]
        chat = f64(chat)
        assert Gd.shape == (n, n) and Hd.shape == (n, n) and chat.shape == (j,)
        self.check(self.lib.lz_os_state_set(self._h, int(j), dptr(Gd), dptr(Hd), dptr(chat), float(alpha_prev), float(beta_prev),
                                            float(beta_prev2)))

    def os_step(self, form, j, wide=False):
        """one single (1), pair (2) or group (4) step at ``j``; returns the block count of the walk it launched"""
        nb = C.c_int()
        self.check(self.lib.lz_os_step(self._h, int(form), int(j), int(bool(wide)), C.byref(nb)))
        return nb.value

    def os_state_get(self, form, j):
        """everything a step leaves on the device, as a dict (``G``, ``H`` indexed ``[row, column]``)"""
        n = self.n
        ldq = (n + 2 + 15) & ~15
        out = {"G": np.empty((n, n)), "H": np.empty((n, n)), "chat": np.empty(n + 1), "g": np.empty(2 * n + 2), "gq": np.empty((4, n + 4)),
               "d": np.empty(4 * ldq + 16), "elog": np.empty(n + 1), "alpha": np.empty(n + 1), "beta": np.empty(n + 1), "nrm2": np.empty(1),
               "r2": np.empty(self.rows)}
        ist = np.empty(8, dtype=np.int32)
        ldg, ldp = C.c_int(), C.c_int()
        iptr = ist.ctypes.data_as(C.POINTER(C.c_int))
        self.check(self.lib.lz_os_state_get(self._h, int(form), int(j), *[dptr(v) for v in out.values()], iptr, C.byref(ldg), C.byref(ldp)))
        out["G"], out["H"] = out["G"].T.copy(), out["H"].T.copy()
        out.update(ist=ist, ldg=ldg.value, ldp=ldp.value)
        return out

    def os_raw_get(self, j0, count, part_count):
        """rows ``j0 .. j0 + count - 1`` with their padding, and the first ``part_count`` partial sums the last step's walk wrote"""
        rows = np.empty((count, self.padded_rows(self.rows)))
        part = np.empty(part_count)
        self.check(self.lib.lz_os_raw_get(self._h, int(j0), int(count), dptr(rows), dptr(part), int(part_count)))
        return rows, part

    # ---- two-sided (bi-orthogonal) Lanczos ----
    def set_csr_transpose(self, rowptr=None, colidx=None, vals=None):
        """``None``: H is symmetric (H^T x runs on H)."""
        if rowptr is None:
            self.check(self.lib.lz_set_csr_transpose(self._h, 0, None, None, None))
            return
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
        colidx = np.ascontiguousarray(colidx, dtype=np.int32)
        vals = f64(vals)
        self.check(self.lib.lz_set_csr_transpose(self._h, int(rowptr[-1]), i32ptr(rowptr), i32ptr(colidx), dptr(vals)))

    def run_two_sided(self, n, q0, p0):
        q0, p0 = f64(q0), f64(p0)
        if q0.shape != (self.rows,) or p0.shape != (self.rows,):
            raise ValueError("start pair has the wrong length")
        alpha, beta, gamma = np.zeros(n), np.zeros(max(n - 1, 1)), np.zeros(max(n - 1, 1))
        self.check(self.lib.lz_run_two_sided(self._h, int(n), dptr(q0), dptr(p0), dptr(alpha), dptr(beta), dptr(gamma)))
        self.n = n
        return alpha, beta[: n - 1], gamma[: n - 1]

    def bi_alloc(self, n):
        self.check(self.lib.lz_bi_alloc(self._h, int(n)))
        self.n = n

    def bi_set_row(self, which, j, row):
        row = f64(row)
        assert row.shape == (self.rows,)
        self.check(self.lib.lz_bi_set_row(self._h, int(which), int(j), dptr(row)))

    def bi_get_row(self, which, j):
        out = np.empty(self.rows)
        self.check(self.lib.lz_bi_get_row(self._h, int(which), int(j), dptr(out)))
        return out

    def step_bireorth(self, j):
        self.check(self.lib.lz_step_bireorth(self._h, int(j)))

    def step_bireorth_mem_safe(self, j):
        self.check(self.lib.lz_step_bireorth_mem_safe(self._h, int(j)))

    # -- thick-restart Lanczos (lanczos_amd.eigsh): a basis of its own, never the fixed-n run's V / Y
    def trl_begin(self, m, v0):
        self.trl_m, self.trl_b = int(m), 1
        self.check(self.lib.lz_trl_begin(self._h, int(m), dptr(f64(v0))))

    def trl_extend(self, k, m):
        """steps k .. m-1 -> (proj (m, m): row j = T[0..j, j] for j >= k, beta (m,))"""
        proj = np.zeros((m, m))
        beta = np.zeros(m)
        self.check(self.lib.lz_trl_extend(self._h, int(k), int(m), dptr(proj), dptr(beta)))
        return proj, beta

    def trl_begin_band(self, m, X):
        """band Lanczos: a basis of m + b rows, rows 0 .. b-1 from the b rows of X (orthonormalised one by one)"""
        X = f64(X)
        assert X.ndim == 2 and X.shape[1] == self.rows
        self.trl_m, self.trl_b = int(m), X.shape[0]
        self.check(self.lib.lz_trl_begin_band(self._h, int(m), X.shape[0], dptr(X)))

    def trl_extend_band(self, k, m):
        """steps k .. m-1 -> (proj (m, m + b): row j = the coefficients of A V[j] on V[0 .. j + b) for j >= k, beta (m,))"""
        proj = np.zeros((m, m + self.trl_b))
        beta = np.zeros(m)
        self.check(self.lib.lz_trl_extend_band(self._h, int(k), int(m), dptr(proj), dptr(beta)))
        return proj, beta

    def trl_restart(self, m, kk, S):
        S = f64(S)
        assert S.shape == (m, kk)
        self.check(self.lib.lz_trl_restart(self._h, int(m), int(kk), dptr(S)))

    def trl_probe(self, k, x):
        self.check(self.lib.lz_trl_probe(self._h, int(k), dptr(f64(x))))

    def trl_get_vectors(self, k):
        Y = np.empty((self.rows, int(k)))
        self.check(self.lib.lz_trl_get_vectors(self._h, int(k), dptr(Y)))
        return Y

    def trl_residuals(self, k, theta):
        th = f64(theta)[: int(k)]
        out = np.empty(int(k))
        self.check(self.lib.lz_trl_residuals(self._h, int(k), dptr(th), dptr(out)))
        return out

    def trl_residuals_cplx(self, k, re, im):
        """|A x - (re + i im) x| for eigenvectors in real form in rows 0 .. k-1 (a pair: rows i, i + 1 = Re x, Im x; both get its norm)"""
        re, im = f64(re)[: int(k)], f64(im)[: int(k)]
        assert re.shape == (int(k),) and im.shape == (int(k),)
        out = np.empty(int(k))
        self.check(self.lib.lz_trl_residuals_cplx(self._h, int(k), dptr(re), dptr(im), dptr(out)))
        return out

    def trl_set_filter(self, coefficients, c=0.0):
        """coefficients: the (a_i, b_i) pairs of ``ChebFilter.coefficients()``; None or empty switches the filter off"""
        ab = np.zeros((0, 2)) if coefficients is None else f64(coefficients).reshape(-1, 2)
        a, b = f64(ab[:, 0].copy()), f64(ab[:, 1].copy())
        self.check(self.lib.lz_trl_set_filter(self._h, len(a), dptr(a) if len(a) else None, dptr(b) if len(b) else None, float(c)))

    def trl_set_series(self, coefficients, c=0.0, e=1.0):
        """coefficients: the ``degree + 1`` values of ``SeriesFilter.coefficients()`` on ``[c - e, c + e]``; None or empty clears the series"""
        mu = np.zeros(0) if coefficients is None else f64(coefficients).reshape(-1)
        if len(mu) == 1:
            raise ValueError("a series needs at least two coefficients (degree >= 1)")
        self.check(self.lib.lz_trl_set_series(self._h, max(len(mu) - 1, 0), dptr(mu) if len(mu) else None, float(c), float(e)))

    def trl_filter_apply(self, x):
        """p(A) x (the filter or the series set) through the device kernels; the residual row V[m] is overwritten"""
        x = f64(x)
        assert x.shape == (self.rows,)
        y = np.empty(self.rows)
        self.check(self.lib.lz_trl_filter_apply(self._h, dptr(x), dptr(y)))
        return y

    def trl_rayleigh(self, k):
        """V[0..k) A V[0..k)^T, (k, k)"""
        G = np.empty((int(k), int(k)))
        self.check(self.lib.lz_trl_rayleigh(self._h, int(k), dptr(G)))
        return G

    def trl_set_rows(self, j0, rows):
        """raw basis rows j0 .. j0 + len(rows) - 1 including their padding: rows is (count, >= padded_rows(M))"""
        rows = f64(rows)
        self.check(self.lib.lz_trl_set_rows(self._h, int(j0), rows.shape[0], dptr(rows), rows.shape[1]))

    def trl_get_rows(self, j0, count):
        out = np.empty((int(count), self.padded_rows(self.rows)))
        self.check(self.lib.lz_trl_get_rows(self._h, int(j0), int(count), dptr(out), out.shape[1]))
        return out

    # -- complex Hermitian matrices (lanczos_amd.eigsh on complex input): a matrix and a basis of their own; one matrix at a time - a
    # complex setter drops the real matrix and the other way round
    def set_csr_cplx(self, n, rowptr, colidx, vals):
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
        colidx = np.ascontiguousarray(colidx, dtype=np.int32)
        vals = c128(vals)
        # (SciPy allows ``indices`` / ``data`` longer than ``indptr[-1]``: the entries behind it are not the matrix)
        assert len(rowptr) == int(n) + 1 and min(len(colidx), len(vals)) >= int(rowptr[-1])
        self.check(self.lib.lz_set_csr_cplx(self._h, int(n), int(rowptr[-1]), i32ptr(rowptr), i32ptr(colidx), dptr(vals)))
        self.rows = int(n)
        self.matrix_uploads += 1

    def set_dense_cplx(self, A):
        """row-major complex128; an array that is not C-contiguous is copied (the memory of an F-ordered Hermitian array read by
        rows is the conjugate, not the matrix)"""
        A = c128(A)
        if A.ndim != 2 or A.shape[0] != A.shape[1]:
            raise ValueError("dense H must be square")
        self.check(self.lib.lz_set_dense_cplx(self._h, A.shape[0], dptr(A)))
        self.rows = A.shape[0]
        self.matrix_uploads += 1

    def zspmv(self, x):
        """A x through the complex product kernel, host vectors"""
        x = c128(x)
        assert x.shape == (self.rows,)
        y = np.empty(self.rows, dtype=np.complex128)
        self.check(self.lib.lz_zspmv_host(self._h, dptr(x), dptr(y)))
        return y

    def ztrl_begin(self, m, v0):
        v0 = c128(v0)
        assert v0.shape == (self.rows,)
        self.ztrl_m = int(m)
        self.check(self.lib.lz_ztrl_begin(self._h, int(m), dptr(v0)))

    def ztrl_extend(self, k, m):
        """steps k .. m-1 -> (proj (m, m) complex: row j = <V_i, A V[j]> for i <= j, j >= k; beta (m,) real)"""
        proj = np.zeros((m, m), dtype=np.complex128)
        beta = np.zeros(m)
        self.check(self.lib.lz_ztrl_extend(self._h, int(k), int(m), dptr(proj), dptr(beta)))
        return proj, beta

    def ztrl_restart(self, m, kk, S):
        S = c128(S)
        assert S.shape == (m, kk)
        self.check(self.lib.lz_ztrl_restart(self._h, int(m), int(kk), dptr(S)))

    def ztrl_probe(self, k, x):
        x = c128(x)
        assert x.shape == (self.rows,)
        self.check(self.lib.lz_ztrl_probe(self._h, int(k), dptr(x)))

    def ztrl_get_vectors(self, k):
        Y = np.empty((self.rows, int(k)), dtype=np.complex128)
        self.check(self.lib.lz_ztrl_get_vectors(self._h, int(k), dptr(Y)))
        return Y

    def ztrl_residuals(self, k, theta):
        th = f64(theta)[: int(k)]
        assert th.shape == (int(k),)
        out = np.empty(int(k))
        self.check(self.lib.lz_ztrl_residuals(self._h, int(k), dptr(th), dptr(out)))
        return out

    def ztrl_set_rows(self, j0, rows):
        """basis rows j0 .. j0 + len(rows) - 1 from ``rows`` (count, n) complex, unpadded"""
        rows = c128(rows)
        assert rows.ndim == 2 and rows.shape[1] == self.rows
        self.check(self.lib.lz_ztrl_set_rows(self._h, int(j0), rows.shape[0], dptr(rows), rows.shape[1]))

    def ztrl_get_rows(self, j0, count):
        out = np.empty((int(count), self.rows), dtype=np.complex128)
        self.check(self.lib.lz_ztrl_get_rows(self._h, int(j0), int(count), dptr(out), out.shape[1]))
        return out

    # -- matrix exponential action (lanczos_amd.expm_multiply): a basis of its own, real or planar complex, on whichever matrix is set
    def expm_begin(self, m, v0, cplx):
        """``cplx``: the planar complex basis (required on a complex matrix; on a real one it selects the mixed product)"""
        v0 = c128(v0) if cplx else f64(v0)
        assert v0.shape == (self.rows,)
        self.expm_m, self.expm_cplx = int(m), bool(cplx)
        self.check(self.lib.lz_expm_begin(self._h, int(m), 1 if cplx else 0, dptr(v0)))

    def expm_extend(self, k0, k1):
        """steps k0 .. k1-1 -> (proj (m, m): row j = <V_i, A V[j]> for i <= j, written for k0 <= j < k1; beta (m,) real)"""
        m = self.expm_m
        proj = np.zeros((m, m), dtype=np.complex128 if self.expm_cplx else np.float64)
        beta = np.zeros(m)
        self.check(self.lib.lz_expm_extend(self._h, int(k0), int(k1), dptr(proj), dptr(beta)))
        return proj, beta

    def expm_combine(self, mm, Cm):
        """rows ``0 .. ncols-1`` become ``sum_i Cm[i, c] V_i`` over the first ``mm`` rows, row 0 is normalised; returns its norm before that"""
        Cm = c128(Cm) if self.expm_cplx else f64(Cm)
        assert Cm.ndim == 2 and Cm.shape[0] == int(mm)
        nrm = C.c_double()
        self.check(self.lib.lz_expm_combine(self._h, int(mm), Cm.shape[1], dptr(Cm), C.byref(nrm)))
        return nrm.value

    def expm_get_rows(self, j0, count):
        """rows j0 .. j0 + count - 1 as (count, n), without padding"""
        if self.expm_cplx:
            out = np.empty((int(count), self.rows), dtype=np.complex128)
            self.check(self.lib.lz_expm_get_rows(self._h, int(j0), int(count), dptr(out), out.shape[1]))
            return out
        out = np.empty((int(count), self.padded_rows(self.rows)))
        self.check(self.lib.lz_expm_get_rows(self._h, int(j0), int(count), dptr(out), out.shape[1]))
        return np.ascontiguousarray(out[:, : self.rows])

    # -- symmetric linear solves (lanczos_amd.minres): seven vectors of their own on the real matrix set
    MINRES_VECTORS = {"x": 0, "v": 1, "v_prev": 2, "w1": 3, "w2": 4, "r": 5}
    MINRES_STATE = ("iterations", "done", "phibar", "beta1", "anorm", "alpha", "beta", "phi")

    def minres_begin(self, b, x0=None, shift=0.0):
        """``r0 = b - (A - shift I) x0`` (``x0`` None: ``r0 = b``); a fresh state"""
        b = f64(b)
        assert b.shape == (self.rows,)
        if x0 is not None:
            x0 = f64(x0)
            assert x0.shape == (self.rows,)
        self.check(self.lib.lz_minres_begin(self._h, dptr(b), dptr(x0) if x0 is not None else None, float(shift)))

    def minres_run(self, iters, rtol):
        """up to ``iters`` steps with no host synchronisation between them -> ``{"iterations", "done", "phibar", "beta1", "anorm", "alpha",
        "beta", "phi"}`` (the totals and the last step's scalars)"""
        out = np.zeros(8)
        self.check(self.lib.lz_minres_run(self._h, int(iters), float(rtol), dptr(out)))
        st = dict(zip(self.MINRES_STATE, (float(v) for v in out)))
        st["iterations"], st["done"] = int(out[0]), bool(out[1])
        return st

    def minres_history(self, count):
        """``phibar`` after steps ``1 .. count``"""
        out = np.zeros(int(count))
        self.check(self.lib.lz_minres_history(self._h, dptr(out), int(count)))
        return out

    def minres_get(self, which, raw=False):
        """a vector of the state (``"x"``, ``"v"`` = v_k, ``"v_prev"``, ``"w1"`` = w_{k-1}, ``"w2"``, ``"r"``) as ``n`` doubles;
        ``raw``: the padded device vector"""
        out = np.empty(self.padded_rows(self.rows) if raw else self.rows)
        self.check(self.lib.lz_minres_get(self._h, self.MINRES_VECTORS[which] | (8 if raw else 0), dptr(out)))
        return out

    def minres_set_state(self, k, x, vk, vkm1, wkm1, wkm2, scalars):
        """the state step ``k`` starts from; ``scalars`` = (beta_k, cs, sn, dbar, epsln, phibar, tnorm2, beta1, shift)"""
        vecs = [f64(v) for v in (x, vk, vkm1, wkm1, wkm2)]
        assert all(v.shape == (self.rows,) for v in vecs)
        sc = f64(scalars)
        assert sc.shape == (9,)
        self.check(self.lib.lz_minres_set_state(self._h, int(k), *(dptr(v) for v in vecs), dptr(sc)))

    def minres_step_time(self, reps=20):
        """device milliseconds of ``(one product, one k_minres_step)`` of the plan (means of ``reps`` launches); spends the state"""
        out = np.zeros(2)
        self.check(self.lib.lz_minres_step_time(self._h, int(reps), dptr(out)))
        return float(out[0]), float(out[1])

    def minres_info(self):
        """{"launches_per_iteration", "scale_on_read": the product forms v = r / beta as it reads r, "live"}"""
        out = (C.c_int * 3)()
        self.check(self.lib.lz_minres_info(self._h, out))
        return {"launches_per_iteration": int(out[0]), "scale_on_read": bool(out[1]), "live": bool(out[2])}

    # -- non-symmetric linear solves (lanczos_amd.bicgstab): six vectors of their own on the real square matrix set
    BICGSTAB_VECTORS = {"x": 0, "r": 1, "rtilde": 2, "p": 3, "v": 4, "t": 5}
    BICGSTAB_STATE = ("iterations", "done", "code", "exit", "head", "rnorm", "rho", "rho_prev", "alpha", "omega", "beta", "snorm", "rv",
                      "ts", "tt")
    BICGSTAB_EXITS = {0: None, 1: "half", 2: "full", 3: "breakdown"}

    def bicgstab_begin(self, b, x0=None):
        """``r = b - A x0`` (``x0`` None: ``r = b``), ``rtilde = r``; a fresh state whose head tests the first ``bicgstab_run`` applies"""
        b = f64(b)
        assert b.shape == (self.rows,)
        if x0 is not None:
            x0 = f64(x0)
            assert x0.shape == (self.rows,)
        self.check(self.lib.lz_bicgstab_begin(self._h, dptr(b), dptr(x0) if x0 is not None else None))

    def bicgstab_run(self, iters, atol_eff):
        """up to ``iters`` iterations with no host synchronisation between them -> a dict of ``BICGSTAB_STATE`` (the totals, how the
        state ended - ``exit`` is None, ``"half"``, ``"full"`` or ``"breakdown"`` - and the last iteration's scalars)"""
        out = np.zeros(16)
        self.check(self.lib.lz_bicgstab_run(self._h, int(iters), float(atol_eff), dptr(out)))
        st = dict(zip(self.BICGSTAB_STATE, (float(v) for v in out)))
        st["iterations"], st["done"], st["code"], st["head"] = int(out[0]), bool(out[1]), int(out[2]), bool(out[4])
        st["exit"] = self.BICGSTAB_EXITS[int(out[3])]
        return st

    def bicgstab_history(self, count):
        """``(count, 2)``: ``|s|``, ``|r|`` of iterations ``0 .. count - 1``"""
        out = np.zeros((int(count), 2))
        self.check(self.lib.lz_bicgstab_history(self._h, dptr(out), int(count)))
        return out

    def bicgstab_get(self, which, raw=False):
        """a vector of the state (``"x"``, ``"r"``, ``"rtilde"``, ``"p"``, ``"v"``, ``"t"``) as ``n`` doubles; ``raw``: the padded device vector"""
        out = np.empty(self.padded_rows(self.rows) if raw else self.rows)
        self.check(self.lib.lz_bicgstab_get(self._h, self.BICGSTAB_VECTORS[which] | (8 if raw else 0), dptr(out)))
        return out

    def bicgstab_set_state(self, k, x, r, rtilde, p, v, scalars):
        """the state iteration ``k`` (from 0) starts from; ``scalars`` = (rho_prev, alpha, omega)"""
        vecs = [f64(a) for a in (x, r, rtilde, p, v)]
        assert all(a.shape == (self.rows,) for a in vecs)
        sc = f64(scalars)
        assert sc.shape == (3,)
        self.check(self.lib.lz_bicgstab_set_state(self._h, int(k), *(dptr(a) for a in vecs), dptr(sc)))

    def bicgstab_step_time(self, reps=20):
        """device milliseconds of ``(A p, A s, k_bicgstab_p, k_bicgstab_s, k_bicgstab_tt, k_bicgstab_r)`` (means of ``reps`` launches);
        spends the state"""
        out = np.zeros(6)
        self.check(self.lib.lz_bicgstab_step_time(self._h, int(reps), dptr(out)))
        return tuple(float(v) for v in out)

    def bicgstab_info(self):
        """{"launches_per_iteration", "dots_in_product": the products' epilogue yields ``rtilde . v`` and ``t . s``, "live"}"""
        out = (C.c_int * 3)()
        self.check(self.lib.lz_bicgstab_info(self._h, out))
        return {"launches_per_iteration": int(out[0]), "dots_in_product": bool(out[1]), "live": bool(out[2])}

    # -- symmetric positive definite linear solves (lanczos_amd.cg): five vectors of their own on the real square matrix set
    CG_VECTORS = {"x": 0, "r": 1, "p": 2, "q": 3, "d": 4}
    CG_STATE = ("iterations", "done", "code", "exit", "head", "rnorm", "rho", "rho_prev", "alpha", "beta", "pq", "indefinite_at")
    CG_EXITS = {0: None, 1: "converged", 2: "breakdown"}

    def cg_begin(self, b, x0=None, d=None):
        """``r = b - A x0`` (``x0`` None: ``r = b``), ``p = d r`` (``d`` None: ``p = r``); a fresh state whose head test the first
        ``cg_run`` applies"""
        b = f64(b)
        assert b.shape == (self.rows,)
        if x0 is not None:
            x0 = f64(x0)
            assert x0.shape == (self.rows,)
        if d is not None:
            d = f64(d)
            assert d.shape == (self.rows,)
        self.check(self.lib.lz_cg_begin(self._h, dptr(b), dptr(x0) if x0 is not None else None, dptr(d) if d is not None else None))

    def cg_run(self, iters, atol_eff):
        """up to ``iters`` iterations with no host synchronisation between them -> a dict of ``CG_STATE`` (the totals, how the state
        ended - ``exit`` is None, ``"converged"`` or ``"breakdown"`` - and the last iteration's scalars; ``indefinite_at`` is None or
        the first iteration with ``p . q <= 0``)"""
        out = np.zeros(16)
        self.check(self.lib.lz_cg_run(self._h, int(iters), float(atol_eff), dptr(out)))
        st = dict(zip(self.CG_STATE, (float(v) for v in out)))
        st["iterations"], st["done"], st["code"], st["head"] = int(out[0]), bool(out[1]), int(out[2]), bool(out[4])
        st["exit"] = self.CG_EXITS[int(out[3])]
        st["indefinite_at"] = None if out[11] < 0 else int(out[11])
        return st

    def cg_history(self, count):
        """``|r|`` at the head tests of iterations ``0 .. count - 1``"""
        out = np.zeros(int(count))
        self.check(self.lib.lz_cg_history(self._h, dptr(out), int(count)))
        return out

    def cg_get(self, which, raw=False):
        """a vector of the state (``"x"``, ``"r"``, ``"p"``, ``"q"``, ``"d"``) as ``n`` doubles; ``raw``: the padded device vector"""
        out = np.empty(self.padded_rows(self.rows) if raw else self.rows)
        self.check(self.lib.lz_cg_get(self._h, self.CG_VECTORS[which] | (8 if raw else 0), dptr(out)))
        return out

    def cg_set_state(self, k, x, r, p, d, scalars):
        """the state iteration ``k`` (from 0) starts from: ``p`` is already ``p_k``; ``d`` may be None; ``scalars`` = (rho,)"""
        vecs = [f64(a) for a in (x, r, p)]
        assert all(a.shape == (self.rows,) for a in vecs)
        if d is not None:
            d = f64(d)
            assert d.shape == (self.rows,)
        sc = f64(scalars)
        assert sc.shape == (1,)
        self.check(self.lib.lz_cg_set_state(self._h, int(k), *(dptr(a) for a in vecs), dptr(d) if d is not None else None, dptr(sc)))

    def cg_step_time(self, reps=20):
        """device milliseconds of ``(A p, k_cg_r, k_cg_p)`` (means of ``reps`` launches); spends the state"""
        out = np.zeros(3)
        self.check(self.lib.lz_cg_step_time(self._h, int(reps), dptr(out)))
        return tuple(float(v) for v in out)

    def cg_info(self):
        """{"launches_per_iteration", "preconditioned": the live state has a diagonal ``d``, "live"}"""
        out = (C.c_int * 3)()
        self.check(self.lib.lz_cg_info(self._h, out))
        return {"launches_per_iteration": int(out[0]), "preconditioned": bool(out[1]), "live": bool(out[2])}

    # -- restarted GMRES (lanczos_amd.gmres): a basis of restart + 1 rows, x and b of their own on the real square matrix set
    GMRES_WHICH = {"x": 0, "w": 1, "b": 2, "y": 3, "rows": 4, "small": 5}
    GMRES_STATE = ("iterations", "done", "converged", "breakdown", "inner", "cols", "cycles", "presid", "ptol", "factor", "rnorm", "bnorm",
                   "hcol")
    GMRES_SCALARS = ("cols", "ptol", "factor", "presid", "rnorm", "bnorm", "inner", "breakdown", "done", "converged", "iters", "cycles")

    def gmres_begin(self, restart, b, x0=None):
        """``r = b - A x0`` (``x0`` None: ``r = b``) and ``|b|``; a fresh state whose first test the first ``gmres_run`` applies"""
        b = f64(b)
        assert b.shape == (self.rows,)
        if x0 is not None:
            x0 = f64(x0)
            assert x0.shape == (self.rows,)
        self.check(self.lib.lz_gmres_begin(self._h, int(restart), dptr(b), dptr(x0) if x0 is not None else None))
        self._gmres_m = int(restart)

    def _gmres_st(self, out):
        st = dict(zip(self.GMRES_STATE, (float(v) for v in out)))
        for k in ("iterations", "cols", "cycles", "hcol"):
            st[k] = int(st[k])
        for k in ("done", "converged", "breakdown", "inner"):
            st[k] = bool(st[k])
        return st

    def gmres_run(self, steps, atol_eff):
        """up to ``steps`` inner steps, cycle ends and restarts included, with no host synchronisation between them -> a dict of
        ``GMRES_STATE``"""
        out = np.zeros(16)
        self.check(self.lib.lz_gmres_run(self._h, int(steps), float(atol_eff), dptr(out)))
        return self._gmres_st(out)

    def gmres_end_cycle(self, atol_eff):
        """the end of the cycle under way whatever its length -> a dict of ``GMRES_STATE``"""
        out = np.zeros(16)
        self.check(self.lib.lz_gmres_end_cycle(self._h, float(atol_eff), dptr(out)))
        return self._gmres_st(out)

    def gmres_history(self, count, ncycles):
        """``(presid of inner steps 0 .. count - 1, (ncycles, 3): rnorm, cols, ptol of every cycle)``"""
        hist, cyc = np.zeros(int(count)), np.zeros((int(ncycles), 3))
        self.check(self.lib.lz_gmres_history(self._h, dptr(hist) if count else None, int(count), dptr(cyc) if ncycles else None, int(ncycles)))
        return hist, cyc

    def gmres_get(self, which, raw=False):
        """``"x"``, ``"w"``, ``"b"`` (``n`` doubles; ``raw``: the padded device vector), ``"y"`` (restart), ``"rows"`` (``(restart + 1,
        padded n)``) or ``"small"``: a dict of ``R`` (row ``j`` is column ``j`` of the triangle), ``gc``, ``gs``, ``S``, ``GMRES_SCALARS`` and the
        last step's inputs to k_gmres_column: ``proj``, ``h1``, ``h0sq`` (index ``j``: of the step that made column ``j``)"""
        m, pad = self._gmres_m, self.padded_rows(self.rows)
        w = self.GMRES_WHICH[which]
        if w <= 2:
            out = np.empty(pad if raw else self.rows)
        elif which == "y":
            out = np.empty(m)
        elif which == "rows":
            out = np.empty((m + 1, pad))
        else:
            out = np.empty(m * m + 5 * m + 14)
        self.check(self.lib.lz_gmres_get(self._h, w | (8 if raw and w <= 2 else 0), dptr(out)))
        if which != "small":
            return out
        small = {"R": out[: m * m].reshape(m, m).copy(), "gc": out[m * m: m * m + m].copy(), "gs": out[m * m + m: m * m + 2 * m].copy(),
                 "S": out[m * m + 2 * m: m * m + 3 * m + 1].copy()}
        small.update(zip(self.GMRES_SCALARS, (float(v) for v in out[m * m + 3 * m + 1:])))
        tail = out[m * m + 3 * m + 13:]
        small.update({"proj": tail[:m].copy(), "h1": float(tail[m]), "h0sq": tail[m + 1:].copy()})
        return small

    def gmres_set_state(self, restart, x, b, w, rows, small):
        """upload a whole state: ``x``, ``b`` (``n``), ``w`` (``n`` or padded), basis rows (``(nrows, n)`` or padded), ``small`` as
        ``gmres_get("small")`` returns it"""
        m, pad = int(restart), self.padded_rows(self.rows)
        x, b = f64(x), f64(b)
        assert x.shape == (self.rows,) and b.shape == (self.rows,)
        wp = np.zeros(pad)
        wp[: len(w)] = w
        rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
        rp = np.zeros((rows.shape[0], pad))
        rp[:, : rows.shape[1]] = rows
        packed = np.concatenate([np.asarray(small["R"], dtype=np.float64).reshape(m * m), f64(small["gc"]), f64(small["gs"]), f64(small["S"]),
                                 np.array([float(small[k]) for k in self.GMRES_SCALARS])])
        assert packed.shape == (m * m + 3 * m + 13,)
        self.check(self.lib.lz_gmres_set_state(self._h, m, dptr(x), dptr(b), dptr(wp), dptr(rp), int(rp.shape[0]), dptr(packed)))
        self._gmres_m = m

    def gmres_step_time(self, reps=20):
        """device milliseconds of ``(A V[cols - 1], the Gram-Schmidt step at cols rows, k_gmres_update, launch_trl_cgs at cols rows,
        k_gmres_residual)`` (means of ``reps`` launches); spends the state"""
        out = np.zeros(5)
        self.check(self.lib.lz_gmres_step_time(self._h, int(reps), dptr(out)))
        return tuple(float(v) for v in out)

    def gmres_info(self):
        """{"launches_per_step", "launches_per_cycle_end", "live", "restart"}"""
        out = (C.c_int * 4)()
        self.check(self.lib.lz_gmres_info(self._h, out))
        return {"launches_per_step": int(out[0]), "launches_per_cycle_end": int(out[1]), "live": bool(out[2]), "restart": int(out[3])}

    # -- least-squares solves (lanczos_amd.lsmr): seven vectors of their own on the rectangular (gk) matrix; A is that matrix (p x q) or,
    # with ``transposed``, its transpose
    LSMR_VECTORS = {"x": 0, "u": 1, "v": 2, "h": 3, "hbar": 4}
    LSMR_STATE = ("iterations", "done", "istop", "normr", "normar", "normA", "condA", "normx", "alpha", "beta", "rho", "rhobar", "zeta",
                  "zetabar", "normx_lagged", "normb")
    LSMR_SCALARS = ("alpha", "beta", "alphabar", "rho", "rhobar", "cbar", "sbar", "zeta", "zetabar", "betadd", "betad", "rhodold",
                    "tautildeold", "thetatilde", "d", "normA2", "maxrbar", "minrbar", "damp", "normb", "c1", "c2", "c3")

    def _lsmr_lengths(self, transposed):
        """(length of b, length of x) for ``A`` = the gk matrix or its transpose"""
        p, q = self.gk_shape
        return (q, p) if transposed else (p, q)

    def lsmr_begin(self, b, x0=None, damp=0.0, transposed=False):
        """``u = b - A x0`` (``x0`` None: ``u = b``), ``v = A^T u``; a fresh state with the empty pending update"""
        nb, nx = self._lsmr_lengths(transposed)
        b = f64(b)
        assert b.shape == (nb,)
        if x0 is not None:
            x0 = f64(x0)
            assert x0.shape == (nx,)
        self.lsmr_transposed = bool(transposed)
        self.check(self.lib.lz_lsmr_begin(self._h, 1 if transposed else 0, dptr(b), dptr(x0) if x0 is not None else None, float(damp)))

    def lsmr_run(self, iters, atol, btol, conlim):
        """up to ``iters`` steps with no host synchronisation between them -> a dict of ``LSMR_STATE`` (the totals, the estimates and
        the last step's scalars; ``normx`` is the norm of the ``x`` now held)"""
        out = np.zeros(16)
        self.check(self.lib.lz_lsmr_run(self._h, int(iters), float(atol), float(btol), float(conlim), dptr(out)))
        st = dict(zip(self.LSMR_STATE, (float(v) for v in out)))
        st["iterations"], st["done"], st["istop"] = int(out[0]), bool(out[1]), int(out[2])
        return st

    def lsmr_history(self, count):
        """``(count, 2)``: ``normr``, ``normar`` after steps ``1 .. count``"""
        out = np.zeros((int(count), 2))
        self.check(self.lib.lz_lsmr_history(self._h, dptr(out), int(count)))
        return out

    def lsmr_get(self, which, raw=False):
        """a vector of the state (``"x"``, ``"u"`` = u_k, ``"v"`` = v_k, ``"h"``, ``"hbar"``); ``raw``: the padded device vector"""
        nb, nx = self._lsmr_lengths(self.lsmr_transposed)
        n = nb if which == "u" else nx
        out = np.empty(self.padded_rows(n) if raw else n)
        self.check(self.lib.lz_lsmr_get(self._h, self.LSMR_VECTORS[which] | (8 if raw else 0), dptr(out)))
        return out

    def lsmr_set_state(self, k, x, u, v, hvec, hbar, scalars, transposed=False):
        """the state step ``k`` starts from, the update of step ``k - 1`` pending; ``scalars``: the 23 of ``LSMR_SCALARS``"""
        nb, nx = self._lsmr_lengths(transposed)
        vecs = [f64(a) for a in (x, u, v, hvec, hbar)]
        assert [a.shape for a in vecs] == [(nx,), (nb,), (nx,), (nx,), (nx,)]
        sc = np.zeros(24)
        sc[:23] = f64(scalars)
        self.lsmr_transposed = bool(transposed)
        self.check(self.lib.lz_lsmr_set_state(self._h, 1 if transposed else 0, int(k), *(dptr(a) for a in vecs), dptr(sc)))

    def lsmr_step_time(self, reps=20):
        """device milliseconds of ``(A v, k_lsmr_u, A^T u, k_lsmr_v)`` (means of ``reps`` launches); spends the state"""
        out = np.zeros(4)
        self.check(self.lib.lz_lsmr_step_time(self._h, int(reps), dptr(out)))
        return tuple(float(v) for v in out)

    def lsmr_info(self):
        """{"own_launches_per_iteration": the solver's launches beside the two products, "live", "transposed"}"""
        out = (C.c_int * 3)()
        self.check(self.lib.lz_lsmr_info(self._h, out))
        return {"own_launches_per_iteration": int(out[0]), "live": bool(out[1]), "transposed": bool(out[2])}

    def zspmv_real(self, x):
        """A x for the real matrix set and a complex x, through the mixed product (in the form ``expm_set_product`` selects), host vectors"""
        x = c128(x)
        assert x.shape == (self.rows,)
        y = np.empty(self.rows, dtype=np.complex128)
        self.check(self.lib.lz_zspmv_real_host(self._h, dptr(x), dptr(y)))
        return y

    def expm_set_product(self, form):
        """the mixed product from now on: 0 automatic, 1 two launches of the real product, 2 the two-plane kernel"""
        self.check(self.lib.lz_expm_set_product(self._h, int(form)))

    def expm_product_time(self, reps=20):
        """device milliseconds of one product ``A V[0]`` of the route (mean of ``reps`` launches); overwrites the work vector"""
        ms = C.c_double()
        self.check(self.lib.lz_expm_product_time(self._h, int(reps), C.byref(ms)))
        return ms.value

    def expm_info(self):
        """{"route": "real" / "mixed" / "complex" (None before ``expm_begin``), "product": None / "two-launch" / "two-plane" - the form
        of the last mixed product -, "group": lanes per row of the two-plane CSR kernel for the CSR matrix set (0: none)}"""
        out = (C.c_int * 3)()
        self.check(self.lib.lz_expm_info(self._h, out))
        return {"route": {0: "real", 1: "mixed", 2: "complex"}.get(out[0]), "product": {1: "two-launch", 2: "two-plane"}.get(out[1]),
                "group": int(out[2])}

    # -- Golub-Kahan-Lanczos (lanczos_amd.svds): a rectangular operator and two bases of their own; side 0 = U (length p), 1 = V (length q)
    def gk_set_csr(self, A, AT):
        """``A`` (p x q, p >= q) and ``AT`` (its transpose) as SciPy CSR with sorted indices"""
        p, q = A.shape
        assert AT.shape == (q, p) and A.nnz == AT.nnz
        arrs = [np.ascontiguousarray(A.indptr, dtype=np.int32), np.ascontiguousarray(A.indices, dtype=np.int32), f64(A.data),
                np.ascontiguousarray(AT.indptr, dtype=np.int32), np.ascontiguousarray(AT.indices, dtype=np.int32), f64(AT.data)]
        self.check(self.lib.lz_gk_set_csr(self._h, int(p), int(q), int(A.nnz), i32ptr(arrs[0]), i32ptr(arrs[1]), dptr(arrs[2]),
                                          i32ptr(arrs[3]), i32ptr(arrs[4]), dptr(arrs[5])))
        self.gk_shape = (int(p), int(q))

    def gk_set_dense(self, S, stored_transposed=False):
        """the operator as one dense row-major float64 array: ``S`` is ``p x q`` (``p >= q``), or ``q x p`` with ``stored_transposed``.
        Rows that are contiguous but further apart than their length (a column slice of a wider array) are passed as they are."""
        S = np.asarray(S)
        if S.ndim != 2:
            raise ValueError(f"expected a matrix (shape={S.shape})")
        R, Cn = S.shape
        if S.dtype != np.float64 or S.strides[1] != 8 or S.strides[0] % 8 or S.strides[0] < 8 * Cn:
            S = f64(S)
        p, q = (Cn, R) if stored_transposed else (R, Cn)
        self.check(self.lib.lz_gk_set_dense(self._h, int(p), int(q), dptr(S), S.strides[0] // 8, 1 if stored_transposed else 0))
        self.gk_shape = (int(p), int(q))

    def gk_plan(self):
        """(kind: 0 CSR / 1 dense, stored transposed, form of ``A x``, form of ``A^T u``): the codes of include/lanczos_hip.h"""
        out = (C.c_int * 4)()
        self.check(self.lib.lz_gk_plan(self._h, out))
        return tuple(out)

    def gk_begin(self, m, v0):
        v0 = f64(v0)
        assert v0.shape == (self.gk_shape[1],)
        self.check(self.lib.lz_gk_begin(self._h, int(m), dptr(v0)))

    def gk_extend(self, k, m):
        """steps k .. m-1 -> (colproj (m, m): row j = the coefficients of A V[j] on U[0..j) for j >= k, alpha (m,), beta (m,))"""
        colproj, alpha, beta = np.zeros((m, m)), np.zeros(m), np.zeros(m)
        self.check(self.lib.lz_gk_extend(self._h, int(k), int(m), dptr(colproj), dptr(alpha), dptr(beta)))
        return colproj, alpha, beta

    def gk_restart(self, m, kk, P, Q):
        P, Q = f64(P), f64(Q)
        assert P.shape == (m, kk) and Q.shape == (m, kk)
        self.check(self.lib.lz_gk_restart(self._h, int(m), int(kk), dptr(P), dptr(Q)))

    def gk_probe(self, side, k, x):
        x = f64(x)
        assert x.shape == (self.gk_shape[int(side)],)
        self.check(self.lib.lz_gk_probe(self._h, int(side), int(k), dptr(x)))

    def gk_get_vectors(self, side, k):
        out = np.empty((self.gk_shape[int(side)], int(k)))
        self.check(self.lib.lz_gk_get_vectors(self._h, int(side), int(k), dptr(out)))
        return out

    def gk_set_rows(self, side, j0, rows):
        """raw rows j0 .. j0 + len(rows) - 1 of a basis including their padding: rows is (count, >= padded_rows(p or q))"""
        rows = f64(rows)
        self.check(self.lib.lz_gk_set_rows(self._h, int(side), int(j0), rows.shape[0], dptr(rows), rows.shape[1]))

    def gk_get_rows(self, side, j0, count):
        out = np.empty((int(count), self.padded_rows(self.gk_shape[int(side)])))
        self.check(self.lib.lz_gk_get_rows(self._h, int(side), int(j0), int(count), dptr(out), out.shape[1]))
        return out

    def gk_residuals(self, k, sigma):
        """(2, k): |A v_i - sigma_i u_i| and |A^T u_i - sigma_i v_i|"""
        sg = f64(sigma)[: int(k)]
        out = np.empty((2, int(k)))
        self.check(self.lib.lz_gk_residuals(self._h, int(k), dptr(sg), dptr(out)))
        return out

    def gk_spmv(self, x, transpose=False):
        """one product through the rectangular kernel; the result includes the padding (``padded_rows`` doubles)"""
        x = f64(x)
        p, q = self.gk_shape
        assert x.shape == ((p,) if transpose else (q,))
        y = np.empty(self.padded_rows(q if transpose else p))
        self.check(self.lib.lz_gk_spmv(self._h, 1 if transpose else 0, dptr(x), dptr(y)))
        return y

    def gk_spmv_time(self, transpose=False, reps=20):
        """device milliseconds of one product (mean of ``reps`` launches)"""
        ms = C.c_double()
        self.check(self.lib.lz_gk_spmv_time(self._h, 1 if transpose else 0, int(reps), C.byref(ms)))
        return ms.value

    def spmv_host(self, x, ncols=None):
        x = f64(x)
        y = np.empty(self.rows)
        self.check(self.lib.lz_spmv_host(self._h, dptr(x), dptr(y)))
        return y
