"""krylov.jl_amd -- host-side mirror of Krylov.jl's workspace / solver / operator API over the
MI355X-native C ABI (include/krylov_hip.h, libkrylov_hip.so).

The directory name contains a dot, so import it through the repo-root shim::

    import krylov_jl_amd as K

Naming follows the reference with Python's trailing-underscore convention for Julia's `!`:
`cg!` -> `cg_`, `kaxpy!` -> `kaxpy_`, ...  (src/krylov_utils.jl:305-349, src/cg.jl:120,
src/gmres.jl:121, src/bicgstab.jl:125, src/block_gmres.jl:110).

There is NO CPU fallback: every call goes to hand-written gfx950 kernels; loading fails loudly if
the extension is missing and context creation fails loudly if no GPU is visible.

PyTorch is optional plumbing.  If it is used in the same process (torch.distributed launchers),
import torch BEFORE this package so that both share one HIP runtime (same SONAME libamdhip64.so.7).
"""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess
import sys
import time

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KHIP_LIBRARY") or os.path.join(_HERE, "libkrylov_hip.so")

c_double_p = C.POINTER(C.c_double)
c_void_pp = C.POINTER(C.c_void_p)

APPLY_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)
CALLBACK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p)
GROW_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p)      # khip_grow_fn: push!(V, similar(x)) of an adopted workspace


class KhipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libkrylov_hip error {code}: {msg}")
        self.code = code


class COperator(C.Structure):
    _fields_ = [("csr", C.c_void_p), ("apply", APPLY_FN), ("self", C.c_void_p)]


class COptions(C.Structure):
    _fields_ = [("atol", C.c_double), ("rtol", C.c_double), ("itmax", C.c_int), ("timemax", C.c_double),
                ("history", C.c_int), ("radius", C.c_double), ("linesearch", C.c_int), ("restart", C.c_int),
                ("reorthogonalization", C.c_int), ("fused", C.c_int), ("callback", CALLBACK_FN),
                ("callback_data", C.c_void_p), ("variant", C.c_int), ("verbose", C.c_int), ("log_fd", C.c_int)]


class CMinresParams(C.Structure):
    _fields_ = [("lambda_", C.c_double), ("etol", C.c_double), ("conlim", C.c_double)]


class CSymmlqParams(C.Structure):
    _fields_ = [("lambda_", C.c_double), ("lambda_est", C.c_double), ("etol", C.c_double), ("conlim", C.c_double),
                ("transfer_to_cg", C.c_int)]


class CMinresQlpParams(C.Structure):
    _fields_ = [("lambda_", C.c_double), ("Artol", C.c_double)]


class CLanczosShiftParams(C.Structure):
    _fields_ = [("shifts", c_double_p), ("nshifts", C.c_int), ("check_curvature", C.c_int)]


class CBilqParams(C.Structure):
    _fields_ = [("transfer_to_bicg", C.c_int), ("Mt", C.POINTER(COperator)), ("Nt", C.POINTER(COperator))]


class CQmrParams(C.Structure):
    _fields_ = [("Mt", C.POINTER(COperator)), ("Nt", C.POINTER(COperator))]


class CBilqrParams(C.Structure):
    _fields_ = [("transfer_to_bicg", C.c_int)]


class CUsymlqParams(C.Structure):
    _fields_ = [("transfer_to_usymcg", C.c_int)]


class CTrilqrParams(C.Structure):
    _fields_ = [("transfer_to_usymcg", C.c_int)]


class CTricgParams(C.Structure):
    _fields_ = [("tau", C.c_double), ("nu", C.c_double), ("spd", C.c_int), ("snd", C.c_int), ("flip", C.c_int)]


class CTrimrParams(C.Structure):
    _fields_ = [("tau", C.c_double), ("nu", C.c_double), ("spd", C.c_int), ("snd", C.c_int), ("flip", C.c_int), ("sp", C.c_int)]


class CUsymlqrParams(C.Structure):
    _fields_ = [("ls", C.c_int), ("ln", C.c_int)]


class CStats(C.Structure):
    _fields_ = [("niter", C.c_int), ("solved", C.c_int), ("inconsistent", C.c_int), ("indefinite", C.c_int),
                ("npcCount", C.c_int), ("timer", C.c_double), ("status", C.c_char * 96),
                ("residuals", c_double_p), ("nres", C.c_int), ("error", C.c_char * 160), ("allocation_timer", C.c_double)]


# every symbol include/krylov_hip.h declares: name -> (restype, argtypes)
_i64, _int, _dbl, _vp, _sz = C.c_int64, C.c_int, C.c_double, C.c_void_p, C.c_size_t
SIGNATURES = {
    "khip_last_error": (C.c_char_p, []),
    "khip_version": (None, [C.POINTER(_int), C.POINTER(_int)]),
    "khip_ctx_create": (_int, [_int, _vp, c_void_pp]),
    "khip_ctx_destroy": (_int, [_vp]),
    "khip_ctx_sync": (_int, [_vp]),
    "khip_ctx_stream": (_vp, [_vp]),
    "khip_ctx_set_option": (_int, [_vp, C.c_char_p, _int]),
    "khip_ctx_get_option": (_int, [_vp, C.c_char_p, C.POINTER(_int)]),
    "khip_malloc": (_int, [_vp, _sz, c_void_pp]),
    "khip_free": (_int, [_vp, _vp]),
    "khip_memcpy_h2d": (_int, [_vp, _vp, _vp, _sz]),
    "khip_memcpy_d2h": (_int, [_vp, _vp, _vp, _sz]),
    "khip_memcpy_d2d": (_int, [_vp, _vp, _vp, _sz]),
    "khip_mem_info": (_int, [_vp, C.POINTER(_sz), C.POINTER(_sz)]),
    "khip_csr_create": (_int, [_vp, _i64, _i64, _i64, _vp, _int, _vp, _vp, _int, _int, c_void_pp]),
    "khip_csr_create_dist": (_int, [_vp, _i64, _i64, _i64, _i64, _vp, _int, _vp, _vp, _int, _int, c_void_pp]),
    "khip_csr_destroy": (_int, [_vp]),
    "khip_csr_transpose": (_int, [_vp, _vp, c_void_pp]),
    "khip_csr_compress": (_int, [_vp, _vp, C.POINTER(_int)]),
    "khip_spmv_bytes_stored": (_int, [_vp, C.POINTER(_i64)]),
    "khip_csr_shape": (_int, [_vp, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
    "khip_gen_stencil": (_int, [_vp, _int, _int, _int, _int, _i64, _i64, c_void_pp, c_void_pp, c_void_pp,
                                C.POINTER(_i64)]),
    "khip_gen_banded_random": (_int, [_vp, _i64, _int, _int, C.c_uint64, _int, _int, _i64, _i64, c_void_pp, c_void_pp, c_void_pp,
                                      C.POINTER(_i64)]),
    "khip_spmv": (_int, [_vp, _vp, _vp, _vp]),
    "khip_spmm": (_int, [_vp, _vp, _vp, _vp, _int]),
    "khip_spmv_bytes": (_int, [_vp, C.POINTER(_i64)]),
    "khip_csr_code_info": (_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "khip_csr_sell_info": (_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(_i64)]),
    "khip_csr_sell32_info": (_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(_i64)]),
    "khip_csr_sell_narrow": (_int, [_vp, C.POINTER(C.c_int)]),
    "khip_csr_sell_entries": (_int, [_vp, C.POINTER(C.c_int)]),
    "khip_spmv_kernel_info": (_int, [_vp, _vp, C.POINTER(C.c_int)]),
    "khip_csr_delta_info": (_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(_i64)]),
    "khip_csr_tile_info": (_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int64),
                                  C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "khip_csr_halo_info": (_int, [_vp, C.POINTER(C.c_int), C.POINTER(_i64), C.POINTER(_i64)]),
    "khip_profile_spmv": (_int, [_vp, C.POINTER(_i64), C.POINTER(_dbl)]),
    "khip_profile_kernels": (_int, [_vp, _int, C.POINTER(_i64), C.POINTER(_dbl)]),
    "khip_dot": (_int, [_vp, _i64, _vp, _vp, c_double_p]),
    "khip_nrm2": (_int, [_vp, _i64, _vp, c_double_p]),
    "khip_scal": (_int, [_vp, _i64, _dbl, _vp]),
    "khip_div": (_int, [_vp, _i64, _vp, _dbl]),
    "khip_copy": (_int, [_vp, _i64, _vp, _vp]),
    "khip_scalcopy": (_int, [_vp, _i64, _vp, _dbl, _vp]),
    "khip_divcopy": (_int, [_vp, _i64, _vp, _vp, _dbl]),
    "khip_axpy": (_int, [_vp, _i64, _dbl, _vp, _vp]),
    "khip_axpby": (_int, [_vp, _i64, _dbl, _vp, _dbl, _vp]),
    "khip_fill": (_int, [_vp, _i64, _vp, _dbl]),
    "khip_ref": (_int, [_vp, _i64, _vp, _vp, _dbl, _dbl]),
    "khip_vmul": (_int, [_vp, _i64, _vp, _vp, _vp]),
    "khip_vdiv": (_int, [_vp, _i64, _vp, _vp, _vp]),
    "khip_csr_diagonal": (_int, [_vp, _vp, _vp]),
    "khip_jacobi_create": (_int, [_vp, _vp, C.POINTER(COperator)]),
    "khip_jacobi_destroy": (_int, [C.POINTER(COperator)]),
    "khip_ilu0_create": (_int, [_vp, _vp, C.POINTER(COperator)]),
    "khip_ilu0_destroy": (_int, [C.POINTER(COperator)]),
    "khip_ilu0_info": (_int, [C.POINTER(COperator), C.POINTER(_i64), C.POINTER(_i64), c_void_pp]),
    "khip_ilu0_set_graph": (_int, [C.POINTER(COperator), _int]),
    "khip_ilu0_block_info": (_int, [C.POINTER(COperator), C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_int)]),
    "khip_test_ilu_blocks_host": (_int, [_i64, C.POINTER(_i64), C.POINTER(C.c_int32), _int, C.POINTER(_i64)]),
    "khip_test_ilu0_paths": (_int, [C.POINTER(COperator), C.POINTER(_i64)]),
    "khip_test_ilu_paths_host": (_int, [_i64, C.POINTER(_i64), C.POINTER(C.c_int32), _int, _int, C.POINTER(_i64), C.POINTER(_i64)]),
    "khip_spmv_dot": (_int, [_vp, _vp, _vp, _vp, c_double_p]),
    "khip_axpy2_dot": (_int, [_vp, _i64, _dbl, _vp, _vp, _vp, _vp, c_double_p]),
    "khip_waxpy": (_int, [_vp, _i64, _vp, _vp, _dbl, _vp]),
    "khip_axpy_sqnorm": (_int, [_vp, _i64, _dbl, _vp, _vp, c_double_p]),
    "khip_cg_setup": (_int, [_vp, _i64, _vp, _vp, _vp, _vp, c_double_p]),
    "khip_cg_update": (_int, [_vp, _i64, _dbl, _dbl, _vp, _vp, _vp]),
    "khip_spmv_dotw": (_int, [_vp, _vp, _vp, _vp, _vp, c_double_p]),
    "khip_spmv_dot2": (_int, [_vp, _vp, _vp, _vp, c_double_p]),
    "khip_bicgstab_sx": (_int, [_vp, _i64, _dbl, _vp, _vp, _vp, _vp, _vp]),
    "khip_bicgstab_xr": (_int, [_vp, _i64, _dbl, _vp, _vp, _vp, _vp, _vp, _vp, c_double_p]),
    "khip_bicgstab_p": (_int, [_vp, _i64, _dbl, _dbl, _vp, _vp, _vp]),
    "khip_dot2": (_int, [_vp, _i64, _vp, _vp, c_double_p]),
    "khip_mgs": (_int, [_vp, _i64, _int, c_void_pp, _vp, c_double_p, c_double_p, _int]),
    "khip_hermitian_lanczos": (_int, [_vp, C.POINTER(COperator), _i64, _vp, _int, _int, _int, _vp, _i64, c_double_p, c_double_p]),
    "khip_arnoldi": (_int, [_vp, C.POINTER(COperator), _i64, _vp, _int, _int, _int, _vp, _i64, c_double_p, c_double_p]),
    "khip_golub_kahan": (_int, [_vp, C.POINTER(COperator), C.POINTER(COperator), _i64, _i64, _vp, _int, _int, _vp, _i64, _vp, _i64,
                                c_double_p, c_double_p]),
    "khip_nonhermitian_lanczos": (_int, [_vp, C.POINTER(COperator), C.POINTER(COperator), _i64, _vp, _vp, _int, _int, _vp, _i64, _vp, _i64,
                                         c_double_p, c_double_p, c_double_p, c_double_p]),
    "khip_saunders_simon_yip": (_int, [_vp, C.POINTER(COperator), C.POINTER(COperator), _i64, _i64, _vp, _vp, _int, _int, _vp, _i64, _vp, _i64,
                                       c_double_p, c_double_p, c_double_p, c_double_p]),
    "khip_montoison_orban": (_int, [_vp, C.POINTER(COperator), C.POINTER(COperator), _i64, _i64, _vp, _vp, _int, _int, _int, _vp, _i64, _vp, _i64,
                                    c_double_p, c_double_p, c_double_p, c_double_p]),
    "khip_multi_axpy": (_int, [_vp, _i64, _int, c_double_p, c_void_pp, _vp]),
    "khip_panel_rows": (_int, [_i64, C.POINTER(_i64)]),
    "khip_panel_from_colmajor": (_int, [_vp, _i64, _int, _vp, _vp]),
    "khip_panel_to_colmajor": (_int, [_vp, _i64, _int, _vp, _vp]),
    "khip_panel_gemm_tn": (_int, [_vp, _i64, _int, _vp, _vp, c_double_p]),
    "khip_panel_gemm_nn": (_int, [_vp, _i64, _int, _dbl, _vp, c_double_p, _dbl, _vp]),
    "khip_panel_mgs": (_int, [_vp, _i64, _int, _int, c_void_pp, _vp, c_double_p, _int]),
    "khip_panel_qr": (_int, [_vp, _i64, _int, _vp, c_double_p]),
    "khip_panel_qr_tau": (_int, [_vp, _i64, _int, _vp, c_double_p, c_double_p]),
    "khip_panel_multi_nn": (_int, [_vp, _i64, _int, _int, C.POINTER(_vp), c_double_p, _dbl, _vp]),
    "khip_panel_norm": (_int, [_vp, _i64, _int, _vp, c_double_p]),
    "khip_comm_unique_id": (_int, [_vp]),
    "khip_comm_init": (_int, [_vp, _int, _int, _vp]),
    "khip_comm_init_local": (_int, [_vp, _int, _int, _int]),
    "khip_comm_rank": (_int, [_vp, C.POINTER(_int), C.POINTER(_int)]),
    "khip_comm_barrier": (_int, [_vp]),
    "khip_device_count": (_int, [C.POINTER(_int)]),
    "khip_device_pci_id": (_int, [_int, C.c_char_p, _sz]),
    "khip_comm_info": (_int, [_vp] + [C.POINTER(_int)] * 5),
    "khip_default_options": (COptions, []),
    "khip_cg_workspace_create": (_int, [_vp, _i64, _i64, c_void_pp]),
    "khip_cg_workspace_adopt": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, c_void_pp]),
    "khip_cg_workspace_adopt_vector": (_int, [_vp, C.c_char_p, _vp]),
    "khip_cg_workspace_destroy": (_int, [_vp]),
    "khip_cg_warm_start": (_int, [_vp, _vp]),
    "khip_cg_solve": (_int, [_vp, C.POINTER(COperator), C.POINTER(COperator), _vp, C.POINTER(COptions)]),
    "khip_cg_solution": (_vp, [_vp]),
    "khip_cg_stats": (C.POINTER(CStats), [_vp]),
    "khip_cg_last_path": (_int, [_vp]),
    "khip_cg_vector": (_vp, [_vp, C.c_char_p]),
    "khip_cg_workspace_bytes": (_sz, [_vp]),
    "khip_gmres_workspace_create": (_int, [_vp, _i64, _i64, _int, c_void_pp]),
    "khip_gmres_workspace_adopt": (_int, [_vp, _i64, _i64, _int, _vp, _vp, c_void_pp, c_void_pp]),
    "khip_gmres_workspace_adopt_vector": (_int, [_vp, C.c_char_p, _vp]),
    "khip_gmres_workspace_adopt_basis": (_int, [_vp, _int, c_void_pp]),
    "khip_gmres_workspace_set_grow": (_int, [_vp, GROW_FN, _vp]),
    "khip_gmres_host_state": (_int, [_vp, _int, c_double_p, c_double_p, c_double_p, c_double_p, C.POINTER(_int), C.POINTER(_int)]),
    "khip_gmres_workspace_destroy": (_int, [_vp]),
    "khip_gmres_warm_start": (_int, [_vp, _vp]),
    "khip_gmres_solve": (_int, [_vp, C.POINTER(COperator), C.POINTER(COperator), C.POINTER(COperator), _vp,
                                C.POINTER(COptions)]),
    "khip_gmres_solution": (_vp, [_vp]),
    "khip_gmres_stats": (C.POINTER(CStats), [_vp]),
    "khip_gmres_last_path": (_int, [_vp]),
    "khip_gmres_workspace_bytes": (_sz, [_vp]),
    "khip_bicgstab_workspace_create": (_int, [_vp, _i64, _i64, c_void_pp]),
    "khip_bicgstab_workspace_adopt": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, c_void_pp]),
    "khip_bicgstab_workspace_adopt_vector": (_int, [_vp, C.c_char_p, _vp]),
    "khip_bicgstab_workspace_destroy": (_int, [_vp]),
    "khip_bicgstab_warm_start": (_int, [_vp, _vp]),
    "khip_bicgstab_solve": (_int, [_vp, C.POINTER(COperator), C.POINTER(COperator), C.POINTER(COperator), _vp, _vp,
                                   C.POINTER(COptions)]),
    "khip_bicgstab_solution": (_vp, [_vp]),
    "khip_bicgstab_stats": (C.POINTER(CStats), [_vp]),
    "khip_bicgstab_last_path": (_int, [_vp]),
    "khip_bicgstab_workspace_bytes": (_sz, [_vp]),
    "khip_minres_default_params": (CMinresParams, []),
    "khip_minres_workspace_create": (_int, [_vp, _i64, _i64, _int, c_void_pp]),
    "khip_minres_workspace_adopt": (_int, [_vp, _i64, _i64, _int, _vp, _vp, _vp, _vp, _vp, _vp, c_void_pp]),
    "khip_minres_workspace_adopt_vector": (_int, [_vp, C.c_char_p, _vp]),
    "khip_minres_workspace_destroy": (_int, [_vp]),
    "khip_minres_warm_start": (_int, [_vp, _vp]),
    "khip_minres_solve": (_int, [_vp, C.POINTER(COperator), C.POINTER(COperator), _vp, C.POINTER(COptions),
                                 C.POINTER(CMinresParams)]),
    "khip_minres_solution": (_vp, [_vp]),
    "khip_minres_stats": (C.POINTER(CStats), [_vp]),
    "khip_minres_histories": (_int, [_vp, C.POINTER(c_double_p), C.POINTER(_int), C.POINTER(c_double_p), C.POINTER(_int)]),
    "khip_minres_last_path": (_int, [_vp]),
    "khip_minres_fused_product": (_int, [_vp]),
    "khip_minres_vector": (_vp, [_vp, C.c_char_p]),
    "khip_minres_workspace_bytes": (_sz, [_vp]),
    "khip_cg_lanczos_shift_default_params": (CLanczosShiftParams, []),
    "khip_cg_lanczos_shift_workspace_create": (_int, [_vp, _i64, _i64, _int, c_void_pp]),
    "khip_cg_lanczos_shift_workspace_adopt": (_int, [_vp, _i64, _i64, _int, _vp, _vp, _vp, c_void_pp, c_void_pp, c_void_pp]),
    "khip_cg_lanczos_shift_workspace_adopt_vector": (_int, [_vp, C.c_char_p, _vp]),
    "khip_cg_lanczos_shift_workspace_destroy": (_int, [_vp]),
    "khip_cg_lanczos_shift_solve": (_int, [_vp, C.POINTER(COperator), C.POINTER(COperator), _vp, C.POINTER(COptions),
                                           C.POINTER(CLanczosShiftParams)]),
    "khip_cg_lanczos_shift_solution": (_vp, [_vp, _int]),
    "khip_cg_lanczos_shift_stats": (C.POINTER(CStats), [_vp]),
    "khip_cg_lanczos_shift_residuals": (_int, [_vp, _int, C.POINTER(c_double_p), C.POINTER(_int)]),
    "khip_cg_lanczos_shift_arrays": (_int, [_vp, c_double_p]),
    "khip_cg_lanczos_shift_last_path": (_int, [_vp]),
    "khip_cg_lanczos_shift_vector": (_vp, [_vp, C.c_char_p]),
    "khip_cg_lanczos_shift_workspace_bytes": (_sz, [_vp]),
    "khip_bilq_default_params": (CBilqParams, []),
    "khip_bilq_workspace_create": (_int, [_vp, _i64, _i64, c_void_pp]),
    "khip_bilq_workspace_adopt": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, c_void_pp]),
    "khip_bilq_workspace_adopt_vector": (_int, [_vp, C.c_char_p, _vp]),
    "khip_bilq_workspace_destroy": (_int, [_vp]),
    "khip_bilq_warm_start": (_int, [_vp, _vp]),
    "khip_bilq_solve": (_int, [_vp, C.POINTER(COperator), C.POINTER(COperator), C.POINTER(COperator), C.POINTER(COperator), _vp, _vp,
                               C.POINTER(COptions), C.POINTER(CBilqParams)]),
    "khip_bilq_solution": (_vp, [_vp]),
    "khip_bilq_stats": (C.POINTER(CStats), [_vp]),
    "khip_bilq_last_path": (_int, [_vp]),
    "khip_bilq_vector": (_vp, [_vp, C.c_char_p]),
    "khip_bilq_workspace_bytes": (_sz, [_vp]),
    "khip_qmr_default_params": (CQmrParams, []),
    "khip_qmr_workspace_create": (_int, [_vp, _i64, _i64, c_void_pp]),
    "khip_qmr_workspace_adopt": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, c_void_pp]),
    "khip_qmr_workspace_adopt_vector": (_int, [_vp, C.c_char_p, _vp]),
    "khip_qmr_workspace_destroy": (_int, [_vp]),
    "khip_qmr_warm_start": (_int, [_vp, _vp]),
    "khip_qmr_solve": (_int, [_vp, C.POINTER(COperator), C.POINTER(COperator), C.POINTER(COperator), C.POINTER(COperator), _vp, _vp,
                              C.POINTER(COptions), C.POINTER(CQmrParams)]),
    "khip_qmr_solution": (_vp, [_vp]),
    "khip_qmr_stats": (C.POINTER(CStats), [_vp]),
    "khip_qmr_last_path": (_int, [_vp]),
    "khip_qmr_vector": (_vp, [_vp, C.c_char_p]),
    "khip_qmr_workspace_bytes": (_sz, [_vp]),
    "khip_usymqr_workspace_create": (_int, [_vp, _i64, _i64, c_void_pp]),
    "khip_usymqr_workspace_adopt": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, c_void_pp]),
    "khip_usymqr_workspace_adopt_vector": (_int, [_vp, C.c_char_p, _vp]),
    "khip_usymqr_workspace_destroy": (_int, [_vp]),
    "khip_usymqr_warm_start": (_int, [_vp, _vp]),
    "khip_usymqr_solve": (_int, [_vp, C.POINTER(COperator), C.POINTER(COperator), _vp, _vp, C.POINTER(COptions)]),
    "khip_usymqr_solution": (_vp, [_vp]),
    "khip_usymqr_stats": (C.POINTER(CStats), [_vp]),
    "khip_usymqr_aresiduals": (_int, [_vp, C.POINTER(c_double_p), C.POINTER(_int)]),
    "khip_usymqr_last_path": (_int, [_vp]),
    "khip_usymqr_vector": (_vp, [_vp, C.c_char_p]),
    "khip_usymqr_workspace_bytes": (_sz, [_vp]),
    "khip_usymlq_default_params": (CUsymlqParams, []),
    "khip_usymlq_workspace_create": (_int, [_vp, _i64, _i64, c_void_pp]),
    "khip_usymlq_workspace_adopt": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, c_void_pp]),
    "khip_usymlq_workspace_adopt_vector": (_int, [_vp, C.c_char_p, _vp]),
    "khip_usymlq_workspace_destroy": (_int, [_vp]),
    "khip_usymlq_warm_start": (_int, [_vp, _vp]),
    "khip_usymlq_solve": (_int, [_vp, C.POINTER(COperator), C.POINTER(COperator), _vp, _vp, C.POINTER(COptions),
                                 C.POINTER(CUsymlqParams)]),
    "khip_usymlq_solution": (_vp, [_vp]),
    "khip_usymlq_stats": (C.POINTER(CStats), [_vp]),
    "khip_usymlq_last_path": (_int, [_vp]),
    "khip_usymlq_vector": (_vp, [_vp, C.c_char_p]),
    "khip_usymlq_workspace_bytes": (_sz, [_vp]),
    "khip_trilqr_default_params": (CTrilqrParams, []),
    "khip_trilqr_workspace_create": (_int, [_vp, _i64, _i64, c_void_pp]),
    "khip_trilqr_workspace_adopt": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, c_void_pp]),
    "khip_trilqr_workspace_adopt_vector": (_int, [_vp, C.c_char_p, _vp]),
    "khip_trilqr_workspace_destroy": (_int, [_vp]),
    "khip_trilqr_warm_start": (_int, [_vp, _vp, _vp]),
    "khip_trilqr_solve": (_int, [_vp, C.POINTER(COperator), C.POINTER(COperator), _vp, _vp, C.POINTER(COptions),
                                 C.POINTER(CTrilqrParams)]),
    "khip_trilqr_solution_x": (_vp, [_vp]),
    "khip_trilqr_solution_y": (_vp, [_vp]),
    "khip_trilqr_stats": (C.POINTER(CStats), [_vp]),
    "khip_trilqr_adjoint_stats": (_int, [_vp, C.POINTER(_int), C.POINTER(_int), C.POINTER(c_double_p), C.POINTER(_int),
                                         C.POINTER(c_double_p), C.POINTER(_int), C.POINTER(C.c_char_p)]),
    "khip_trilqr_last_path": (_int, [_vp]),
    "khip_trilqr_vector": (_vp, [_vp, C.c_char_p]),
    "khip_trilqr_workspace_bytes": (_sz, [_vp]),
    "khip_tricg_default_params": (CTricgParams, []),
    "khip_tricg_workspace_create": (_int, [_vp, _i64, _i64, c_void_pp]),
    "khip_tricg_workspace_adopt": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, c_void_pp]),
    "khip_tricg_workspace_adopt_vector": (_int, [_vp, C.c_char_p, _vp]),
    "khip_tricg_workspace_destroy": (_int, [_vp]),
    "khip_tricg_warm_start": (_int, [_vp, _vp, _vp]),
    "khip_tricg_solve": (_int, [_vp, C.POINTER(COperator), C.POINTER(COperator), _vp, _vp, C.POINTER(COptions),
                                C.POINTER(CTricgParams)]),
    "khip_tricg_solution_x": (_vp, [_vp]),
    "khip_tricg_solution_y": (_vp, [_vp]),
    "khip_tricg_stats": (C.POINTER(CStats), [_vp]),
    "khip_tricg_last_path": (_int, [_vp]),
    "khip_tricg_vector": (_vp, [_vp, C.c_char_p]),
    "khip_tricg_workspace_bytes": (_sz, [_vp]),
    "khip_trimr_default_params": (CTrimrParams, []),
    "khip_trimr_workspace_create": (_int, [_vp, _i64, _i64, c_void_pp]),
    "khip_trimr_workspace_adopt": (_int, [_vp, _i64, _i64] + [_vp] * 16 + [c_void_pp]),
    "khip_trimr_workspace_adopt_vector": (_int, [_vp, C.c_char_p, _vp]),
    "khip_trimr_workspace_destroy": (_int, [_vp]),
    "khip_trimr_warm_start": (_int, [_vp, _vp, _vp]),
    "khip_trimr_solve": (_int, [_vp, C.POINTER(COperator), C.POINTER(COperator), _vp, _vp, C.POINTER(COptions),
                                C.POINTER(CTrimrParams)]),
    "khip_trimr_solution_x": (_vp, [_vp]),
    "khip_trimr_solution_y": (_vp, [_vp]),
    "khip_trimr_stats": (C.POINTER(CStats), [_vp]),
    "khip_trimr_last_path": (_int, [_vp]),
    "khip_trimr_vector": (_vp, [_vp, C.c_char_p]),
    "khip_trimr_workspace_bytes": (_sz, [_vp]),
    "khip_test_trimr_p3": (_int, [_vp, _i64, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "khip_test_trimr_g": (_int, [_vp, _i64, _vp, _vp, _int, _vp, _vp, _vp, _vp, _vp, C.c_double]),
    "khip_usymlqr_default_params": (CUsymlqrParams, []),
    "khip_usymlqr_workspace_create": (_int, [_vp, _i64, _i64, c_void_pp]),
    "khip_usymlqr_workspace_adopt": (_int, [_vp, _i64, _i64] + [_vp] * 13 + [c_void_pp]),
    "khip_usymlqr_workspace_adopt_vector": (_int, [_vp, C.c_char_p, _vp]),
    "khip_usymlqr_workspace_destroy": (_int, [_vp]),
    "khip_usymlqr_warm_start": (_int, [_vp, _vp, _vp]),
    "khip_usymlqr_solve": (_int, [_vp, C.POINTER(COperator), C.POINTER(COperator), _vp, _vp, C.POINTER(COptions),
                                  C.POINTER(CUsymlqrParams)]),
    "khip_usymlqr_solution_x": (_vp, [_vp]),
    "khip_usymlqr_solution_y": (_vp, [_vp]),
    "khip_usymlqr_stats": (C.POINTER(CStats), [_vp]),
    "khip_usymlqr_aresiduals": (_int, [_vp, C.POINTER(c_double_p), C.POINTER(_int)]),
    "khip_usymlqr_last_path": (_int, [_vp]),
    "khip_usymlqr_vector": (_vp, [_vp, C.c_char_p]),
    "khip_usymlqr_workspace_bytes": (_sz, [_vp]),
    "khip_test_usymlqr_p3": (_int, [_vp, _i64, _int, _int, _int] + [_vp] * 14),
    "khip_cgs_workspace_create": (_int, [_vp, _i64, _i64, c_void_pp]),
    "khip_cgs_workspace_adopt": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, c_void_pp]),
    "khip_cgs_workspace_adopt_vector": (_int, [_vp, C.c_char_p, _vp]),
    "khip_cgs_workspace_destroy": (_int, [_vp]),
    "khip_cgs_warm_start": (_int, [_vp, _vp]),
    "khip_cgs_solve": (_int, [_vp, C.POINTER(COperator), C.POINTER(COperator), C.POINTER(COperator), _vp, _vp,
                              C.POINTER(COptions)]),
    "khip_cgs_solution": (_vp, [_vp]),
    "khip_cgs_stats": (C.POINTER(CStats), [_vp]),
    "khip_cgs_last_path": (_int, [_vp]),
    "khip_cgs_vector": (_vp, [_vp, C.c_char_p]),
    "khip_cgs_workspace_bytes": (_sz, [_vp]),
    "khip_symmlq_default_params": (CSymmlqParams, []),
    "khip_symmlq_workspace_create": (_int, [_vp, _i64, _i64, _int, c_void_pp]),
    "khip_symmlq_workspace_adopt": (_int, [_vp, _i64, _i64, _int, _vp, _vp, _vp, _vp, _vp, c_void_pp]),
    "khip_symmlq_workspace_adopt_vector": (_int, [_vp, C.c_char_p, _vp]),
    "khip_symmlq_workspace_destroy": (_int, [_vp]),
    "khip_symmlq_warm_start": (_int, [_vp, _vp]),
    "khip_symmlq_solve": (_int, [_vp, C.POINTER(COperator), C.POINTER(COperator), _vp, C.POINTER(COptions),
                                 C.POINTER(CSymmlqParams)]),
    "khip_symmlq_solution": (_vp, [_vp]),
    "khip_symmlq_stats": (C.POINTER(CStats), [_vp]),
    "khip_symmlq_histories": (_int, [_vp, C.POINTER(c_double_p), C.POINTER(_int), C.POINTER(c_double_p), C.POINTER(_int),
                                     C.POINTER(c_double_p), C.POINTER(_int)]),
    "khip_symmlq_norms": (_int, [_vp, c_double_p, c_double_p]),
    "khip_symmlq_last_path": (_int, [_vp]),
    "khip_symmlq_vector": (_vp, [_vp, C.c_char_p]),
    "khip_symmlq_workspace_bytes": (_sz, [_vp]),
    "khip_minres_qlp_default_params": (CMinresQlpParams, []),
    "khip_minres_qlp_workspace_create": (_int, [_vp, _i64, _i64, c_void_pp]),
    "khip_minres_qlp_workspace_adopt": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, c_void_pp]),
    "khip_minres_qlp_workspace_adopt_vector": (_int, [_vp, C.c_char_p, _vp]),
    "khip_minres_qlp_workspace_destroy": (_int, [_vp]),
    "khip_minres_qlp_warm_start": (_int, [_vp, _vp]),
    "khip_minres_qlp_solve": (_int, [_vp, C.POINTER(COperator), C.POINTER(COperator), _vp, C.POINTER(COptions),
                                     C.POINTER(CMinresQlpParams)]),
    "khip_minres_qlp_solution": (_vp, [_vp]),
    "khip_minres_qlp_stats": (C.POINTER(CStats), [_vp]),
    "khip_minres_qlp_histories": (_int, [_vp, C.POINTER(c_double_p), C.POINTER(_int), C.POINTER(c_double_p), C.POINTER(_int)]),
    "khip_minres_qlp_last_path": (_int, [_vp]),
    "khip_minres_qlp_fused_product": (_int, [_vp]),
    "khip_minres_qlp_vector": (_vp, [_vp, C.c_char_p]),
    "khip_minres_qlp_workspace_bytes": (_sz, [_vp]),
    "khip_bilqr_default_params": (CBilqrParams, []),
    "khip_bilqr_workspace_create": (_int, [_vp, _i64, _i64, c_void_pp]),
    "khip_bilqr_workspace_adopt": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, c_void_pp]),
    "khip_bilqr_workspace_adopt_vector": (_int, [_vp, C.c_char_p, _vp]),
    "khip_bilqr_workspace_destroy": (_int, [_vp]),
    "khip_bilqr_warm_start": (_int, [_vp, _vp, _vp]),
    "khip_bilqr_solve": (_int, [_vp, C.POINTER(COperator), C.POINTER(COperator), _vp, _vp, C.POINTER(COptions),
                                C.POINTER(CBilqrParams)]),
    "khip_bilqr_solution_x": (_vp, [_vp]),
    "khip_bilqr_solution_y": (_vp, [_vp]),
    "khip_bilqr_stats": (C.POINTER(CStats), [_vp]),
    "khip_bilqr_adjoint_stats": (_int, [_vp, C.POINTER(_int), C.POINTER(_int), C.POINTER(c_double_p), C.POINTER(_int),
                                        C.POINTER(c_double_p), C.POINTER(_int), C.POINTER(C.c_char_p)]),
    "khip_bilqr_last_path": (_int, [_vp]),
    "khip_bilqr_vector": (_vp, [_vp, C.c_char_p]),
    "khip_bilqr_workspace_bytes": (_sz, [_vp]),
    "khip_block_gmres_workspace_bytes": (_sz, [_vp, C.POINTER(C.c_size_t)]),
    "khip_test_gen_banded_random_host": (_int, [_i64, _int, _int, C.c_uint64, _int, _int, _i64, _i64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), c_double_p, C.POINTER(_i64)]),
    "khip_test_small_dense": (_int, [_int, _int, _int, _int, c_double_p, c_double_p, c_double_p]),
    "khip_test_deflating_chol": (_int, [_int, c_double_p, C.c_double, _int, C.c_uint, c_double_p, C.POINTER(_int), C.POINTER(C.c_uint)]),
    "khip_test_householder_r": (_int, [_int, _int, c_double_p, c_double_p]),
    "khip_test_householder_signs": (_int, [_int, _i64, c_double_p, c_double_p, c_double_p]),
    "khip_test_optional_build_failures": (_int, [C.POINTER(_int)]),
    "khip_test_csr_arrays": (_int, [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), c_double_p]),
    "khip_test_csr_tile_records": (_int, [_vp, C.POINTER(_i64), c_double_p, _vp, _i64, C.POINTER(C.c_int32), _i64]),
    "khip_test_csr_window_info": (_int, [_vp, C.POINTER(_int), C.POINTER(_i64), C.POINTER(_i64)]),
    "khip_test_spmm_last_launch": (_int, [_vp, C.POINTER(_i64)]),
    "khip_test_set_halo_self": (_int, [_vp, _int]),
    "khip_test_vec_plan": (_int, [_i64, C.POINTER(C.c_uint64), _int, _int, _int, _int, _int, _int, C.POINTER(_i64)]),
    "khip_test_multi_dot": (_int, [_vp, _i64, _int, c_void_pp, _vp, c_double_p]),
    "khip_test_multi_axpy_dev": (_int, [_vp, _i64, _int, c_double_p, c_void_pp, _vp]),
    "khip_test_divcopy_dev": (_int, [_vp, _i64, C.c_double, _vp, _vp]),
    "khip_test_sym_givens": (_int, [C.c_double, C.c_double, c_double_p, c_double_p, c_double_p]),
    "khip_test_bilqr_status": (_int, [_int, C.c_char_p, C.POINTER(C.c_char_p)]),
    "khip_test_roots_quadratic": (_int, [C.c_double, C.c_double, C.c_double, _int, c_double_p, c_double_p]),
    "khip_test_to_boundary": (_int, [_vp, _i64, _vp, _vp, C.c_double, _int, c_double_p, c_double_p]),
    "khip_block_gmres_workspace_create": (_int, [_vp, _i64, _i64, _int, _int, c_void_pp]),
    "khip_block_gmres_workspace_adopt": (_int, [_vp, _i64, _i64, _int, _int, _vp, _vp, c_void_pp, c_void_pp]),
    "khip_block_gmres_workspace_adopt_panel": (_int, [_vp, C.c_char_p, _vp]),
    "khip_block_gmres_workspace_adopt_basis": (_int, [_vp, _int, c_void_pp]),
    "khip_block_gmres_workspace_set_grow": (_int, [_vp, GROW_FN, _vp]),
    "khip_block_gmres_warm_start_panel": (_int, [_vp, _vp]),
    "khip_block_gmres_solve_panel": (_int, [_vp, C.POINTER(COperator), C.POINTER(COperator), C.POINTER(COperator), _vp,
                                     C.POINTER(COptions)]),
    "khip_block_gmres_workspace_destroy": (_int, [_vp]),
    "khip_block_gmres_warm_start": (_int, [_vp, _vp]),
    "khip_block_gmres_solve": (_int, [_vp, C.POINTER(COperator), C.POINTER(COperator), C.POINTER(COperator), _vp,
                               C.POINTER(COptions)]),
    "khip_block_gmres_get_X": (_int, [_vp, _vp]),
    "khip_block_gmres_stats": (C.POINTER(CStats), [_vp]),
    "khip_block_gmres_last_path": (_int, [_vp]),
    # host-only helpers (partition / halo plan logic, testable without a GPU)
    "khip_ghost_columns_host": (_int, [_vp, _vp, _i64, _i64, _vp, _i64, C.POINTER(_i64)]),
    "khip_halo_plan_host": (_int, [_int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _i64]),
}

_lib = None


def build(force: bool = False) -> str:
    """Compile libkrylov_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    script = os.path.join(_HERE, "build.sh")
    srcs = [os.path.join(_HERE, "csrc", f) for f in os.listdir(os.path.join(_HERE, "csrc"))]
    srcs.append(os.path.join(_HERE, "..", "include", "krylov_hip.h"))
    stale = (not os.path.exists(LIB_PATH)) or os.path.getmtime(LIB_PATH) < max(os.path.getmtime(s) for s in srcs)
    if force or stale:
        subprocess.check_call(["bash", script])
    return LIB_PATH


def lib():
    """Load the native library (fails loudly when it is missing: there is no fallback path)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950); krylov.jl_amd has no CPU fallback")
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)      # AttributeError here == header/library mismatch
        fn.restype = res
        fn.argtypes = args
    # khip_options / khip_stats are passed by pointer without a size field: a binding must have been written against the ABI
    # version the library reports; this mirror follows include/krylov_hip.h of version 0.4 (adopt entries, log_fd, last_path)
    major, minor = C.c_int(), C.c_int()
    L.khip_version(C.byref(major), C.byref(minor))
    if (major.value, minor.value) != (0, 4):
        raise ImportError(f"{LIB_PATH} reports ABI {major.value}.{minor.value}; krylov.jl_amd/__init__.py binds 0.4: rebuild (build.sh)")
    _lib = L
    return L


def _ck(rc):
    if rc != 0:
        raise KhipError(rc, lib().khip_last_error().decode("utf-8", "replace"))


def gpu_available() -> bool:
    return os.path.exists("/dev/kfd")


def device_count() -> int:
    n = C.c_int()
    lib().khip_device_count(C.byref(n))
    return n.value


def device_pci_id(device: int = 0) -> str:
    """PCI bus id of the physical GPU behind a visible device index."""
    buf = C.create_string_buffer(64)
    _ck(lib().khip_device_pci_id(device, buf, 64))
    return buf.value.decode()


# --------------------------------------------------------------------------- context / vectors

class Context:
    """Device + HIP stream + reduction scratch (+ RCCL communicator when distributed)."""

    def __init__(self, device: int = 0, stream: int | None = None):
        self._h = C.c_void_p()
        _ck(lib().khip_ctx_create(device, stream, C.byref(self._h)))
        self.device = device
        self.rank, self.nranks = 0, 1

    def close(self):
        if self._h:
            lib().khip_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        _ck(lib().khip_ctx_sync(self._h))

    def set_option(self, key: str, value: int):
        _ck(lib().khip_ctx_set_option(self._h, key.encode(), int(value)))

    def test_set_halo_self(self, enable: int = 1):
        """TEST-ONLY measurement hook (include/krylov_hip_test.h): a one-rank RCCL communicator exchanges its halo with itself."""
        _ck(lib().khip_test_set_halo_self(self._h, int(enable)))

    SPMM_LAUNCH_FIELDS = ("family", "L", "NL", "dbuf", "ahead", "run_len", "grid", "xcd", "launches", "direct", "sweep_S", "sweep_W",
                          "sweep_K", "sweep_cols", "nt", "dist", "p", "pow2", "block", "lds", "num_cu")
    SPMM_FAMILIES = ("none", "spmm_kernel", "spmm2_kernel", "window", "tile1", "tile2")

    def spmm_last_launch(self) -> dict:
        """TEST-ONLY (khip_test_spmm_last_launch): what the last spmm_ on this context launched, family by name."""
        out = (_i64 * 24)()
        _ck(lib().khip_test_spmm_last_launch(self._h, out))
        d = {k: int(out[i]) for i, k in enumerate(self.SPMM_LAUNCH_FIELDS)}
        d["family"] = self.SPMM_FAMILIES[d["family"]]
        return d

    def get_option(self, key: str) -> int:
        v = C.c_int()
        _ck(lib().khip_ctx_get_option(self._h, key.encode(), C.byref(v)))
        return v.value

    def mem_info(self):
        f, t = C.c_size_t(), C.c_size_t()
        _ck(lib().khip_mem_info(self._h, C.byref(f), C.byref(t)))
        return f.value, t.value

    @property
    def stream(self):
        return lib().khip_ctx_stream(self._h)

    def profile_spmv(self):
        """(launches, total_ms) of the SpMV launches recorded since the last call (option profile_spmv=1)."""
        n, ms = C.c_int64(), C.c_double()
        _ck(lib().khip_profile_spmv(self._h, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    PROFILE_TAGS = ("spmv", "spmm", "panel_gemm_tn", "panel_nn_tn", "panel_multi_nn", "panel_gemm_nn", "panel_qr_scale_gram",
                    "halo_pack", "halo_transfer", "dot_allgather_combine", "spmv_boundary", "ssy_p1", "ssy_p2", "usymqr_p3",
                    "usymlq_p3")
    # the families added since: PROFILE_TAGS keeps the length its tests pin (tests/test_usymlq_host.py), profile_kernels reports
    # PROFILE_FAMILIES
    PROFILE_FAMILIES = PROFILE_TAGS + ("trilqr_p3", "tricg_p3", "trimr_p3", "usymlqr_p3")

    def profile_kernels(self):
        """{family: (launches, total_ms)} of the HIP-event brackets recorded since the last call (option profile_spmv = 1):
        khip_profile_kernels -- SpMV, SpMM, the panel kernels of block_gmres! and the fused passes of usymqr!, usymlq!, trilqr!, tricg!, trimr! and usymlqr!."""
        k = len(self.PROFILE_FAMILIES)
        n, ms = (C.c_int64 * k)(), (C.c_double * k)()
        _ck(lib().khip_profile_kernels(self._h, k, n, ms))
        return {t: (int(n[i]), float(ms[i])) for i, t in enumerate(self.PROFILE_FAMILIES)}

    # --- multi-GPU (one process per GPU) ---
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        _ck(lib().khip_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, rank: int, nranks: int, unique_id: bytes):
        assert len(unique_id) == 128
        buf = C.create_string_buffer(unique_id, 128)
        _ck(lib().khip_comm_init(self._h, rank, nranks, buf))
        self.rank, self.nranks = rank, nranks

    def comm_init_local(self, rank: int, nranks: int, hub_id: int = 0):
        """In-process communicator: the ranks are contexts of this process, one host thread each."""
        _ck(lib().khip_comm_init_local(self._h, rank, nranks, hub_id))
        self.rank, self.nranks = rank, nranks

    def comm_info(self) -> dict:
        v = [C.c_int() for _ in range(5)]
        _ck(lib().khip_comm_info(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("rank", "nranks", "rccl_ranks", "local_backend", "halo_comm_separate"), (x.value for x in v)))

    def barrier(self):
        _ck(lib().khip_comm_barrier(self._h))

    # --- allocation helpers ---
    def empty(self, n: int) -> "DeviceVector":
        return DeviceVector(self, n)

    def zeros(self, n: int) -> "DeviceVector":
        v = DeviceVector(self, n)
        kfill_(v, 0.0)
        return v

    def array(self, host) -> "DeviceVector":
        a = np.ascontiguousarray(host, dtype=np.float64).ravel()
        v = DeviceVector(self, a.size)
        v.copy_from_host(a)
        return v


class DeviceVector:
    """Float64 vector in HBM: the storage type `S` of the workspaces (`S(undef, n)`, `similar`,
    `length`; docs/src/custom_workspaces.md:107)."""

    def __init__(self, ctx: Context, n: int, ptr: int | None = None, owner=None):
        self.ctx, self.n = ctx, int(n)
        self._owner = owner
        if ptr is None:
            p = C.c_void_p()
            # pad to a multiple of 2 doubles so 16-byte lane accesses never straddle the allocation
            _ck(lib().khip_malloc(ctx._h, 8 * max(2, (self.n + 1) & ~1), C.byref(p)))
            self.ptr = p.value
            self._owned = True
        else:
            self.ptr = ptr
            self._owned = False

    def __len__(self):
        return self.n

    def similar(self):
        return DeviceVector(self.ctx, self.n)

    def slice(self, lo: int, hi: int) -> "DeviceVector":
        return DeviceVector(self.ctx, hi - lo, ptr=self.ptr + 8 * lo, owner=self)

    def copy_from_host(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64).ravel()
        assert a.size == self.n
        _ck(lib().khip_memcpy_h2d(self.ctx._h, self.ptr, a.ctypes.data, 8 * self.n))
        return self

    def to_host(self) -> np.ndarray:
        out = np.empty(self.n, dtype=np.float64)
        _ck(lib().khip_memcpy_d2h(self.ctx._h, out.ctypes.data, self.ptr, 8 * self.n))
        return out

    def __del__(self):
        try:
            if self._owned and self.ptr and self.ctx._h:
                lib().khip_free(self.ctx._h, self.ptr)
        except Exception:
            pass


def _p(v):
    """device pointer of a DeviceVector / raw int / object with data_ptr() (torch tensor)."""
    if v is None:
        return None
    if isinstance(v, DeviceVector):
        return v.ptr
    if isinstance(v, int):
        return v
    if hasattr(v, "data_ptr"):
        return v.data_ptr()
    raise TypeError(f"not a device buffer: {type(v)}")


# --------------------------------------------------------------------------- k* primitives
# Signatures follow src/krylov_utils.jl:305-349 (n first, scalars as T, return the mutated vector).

def kdot(n, x, y) -> float:
    r = C.c_double()
    _ck(lib().khip_dot(x.ctx._h, n, _p(x), _p(y), C.byref(r)))
    return r.value


kdotr = kdot    # real part; identical for Float64 (src/krylov_utils.jl:313-314)


def knorm(n, x) -> float:
    r = C.c_double()
    _ck(lib().khip_nrm2(x.ctx._h, n, _p(x), C.byref(r)))
    return r.value


def knorm_elliptic(n, x, y) -> float:   # src/krylov_utils.jl:319
    return knorm(n, x) if x is y else math.sqrt(kdotr(n, x, y))


def kscal_(n, s, x):
    _ck(lib().khip_scal(x.ctx._h, n, s, _p(x)))
    return x


def kdiv_(n, x, s):
    _ck(lib().khip_div(x.ctx._h, n, _p(x), s))
    return x


def kcopy_(n, y, x):
    _ck(lib().khip_copy(y.ctx._h, n, _p(y), _p(x)))
    return y


def kscalcopy_(n, y, s, x):
    _ck(lib().khip_scalcopy(y.ctx._h, n, _p(y), s, _p(x)))
    return y


def kdivcopy_(n, y, x, s):
    _ck(lib().khip_divcopy(y.ctx._h, n, _p(y), _p(x), s))
    return y


def kaxpy_(n, s, x, y):
    _ck(lib().khip_axpy(y.ctx._h, n, s, _p(x), _p(y)))
    return y


def kaxpby_(n, s, x, t, y):
    _ck(lib().khip_axpby(y.ctx._h, n, s, _p(x), t, _p(y)))
    return y


def kfill_(x, val):
    _ck(lib().khip_fill(x.ctx._h, x.n, _p(x), val))
    return x


def kref_(n, x, y, c, s):
    _ck(lib().khip_ref(x.ctx._h, n, _p(x), _p(y), c, s))
    return x, y


def kmul_(y, A, x):
    """kmul!(y, A, x) = mul!(y, A, x) (src/krylov_utils.jl:305); A: CsrMatrix, a callable operator, or None (= I,
    the unguarded mul!(v, I, q) of src/bicgstab.jl:222)."""
    if A is None:
        return kcopy_(len(x), y, x)
    if isinstance(A, CsrMatrix):
        _ck(lib().khip_spmv(A.ctx._h, A._h, _p(x), _p(y)))
        return y
    A(x, y)
    return y


def kvmul_(n, w, x, y):
    """w = x .* y (diagonal operator)."""
    _ck(lib().khip_vmul(w.ctx._h, n, _p(w), _p(x), _p(y)))
    return w


def kvdiv_(n, w, x, y):
    """w = x ./ y (Jacobi: z = r ./ diag(A))."""
    _ck(lib().khip_vdiv(w.ctx._h, n, _p(w), _p(x), _p(y)))
    return w


class Jacobi:
    """M = Diagonal(diag(A))^-1 on the device, usable as the M / N argument of cg_ / gmres_ / bicgstab_
    (the reference's Jacobi examples: test/test_gmres.jl:105-128, docs/src/gpu.md)."""

    def __init__(self, A: "CsrMatrix"):
        self.ctx, self.n = A.ctx, A.m
        self.op = COperator()
        _ck(lib().khip_jacobi_create(A.ctx._h, A._h, C.byref(self.op)))

    def __call__(self, x, y):
        return self._apply(x, y)

    def _apply(self, x, y):
        rc = self.op.apply(self.op.self, _p(x), _p(y))
        if rc:
            raise KhipError(rc, lib().khip_last_error().decode())
        return y

    def __del__(self):
        try:
            if self.ctx._h:
                lib().khip_jacobi_destroy(C.byref(self.op))
        except Exception:
            pass


# fused accelerators
def spmv_dot(A, x, y) -> float:
    r = C.c_double()
    _ck(lib().khip_spmv_dot(A.ctx._h, A._h, _p(x), _p(y), C.byref(r)))
    return r.value


def axpy2_dot(n, a, p, q, x, r) -> float:
    out = C.c_double()
    _ck(lib().khip_axpy2_dot(x.ctx._h, n, a, _p(p), _p(q), _p(x), _p(r), C.byref(out)))
    return out.value


def spmv_dotw(A, x, y, w) -> float:
    """y = A x ; returns w . y (src/bicgstab.jl:221-223)."""
    r = C.c_double()
    _ck(lib().khip_spmv_dotw(A.ctx._h, A._h, _p(x), _p(y), _p(w), C.byref(r)))
    return r.value


def spmv_dot2(A, x, y):
    """y = A x ; returns (x . y, y . y) (src/bicgstab.jl:228-230)."""
    out = (C.c_double * 2)()
    _ck(lib().khip_spmv_dot2(A.ctx._h, A._h, _p(x), _p(y), out))
    return out[0], out[1]


def bicgstab_sx_(n, alpha, r, v, y, s, x):
    _ck(lib().khip_bicgstab_sx(x.ctx._h, n, alpha, _p(r), _p(v), _p(y), _p(s), _p(x)))


def bicgstab_xr_(n, omega, s, t, z, c, x, r):
    out = (C.c_double * 2)()
    _ck(lib().khip_bicgstab_xr(x.ctx._h, n, omega, _p(s), _p(t), _p(z), _p(c), _p(x), _p(r), out))
    return out[0], out[1]


def bicgstab_p_(n, omega, beta, v, r, p):
    _ck(lib().khip_bicgstab_p(p.ctx._h, n, omega, beta, _p(v), _p(r), _p(p)))


def axpy_sqnorm(n, a, x, y) -> float:
    """y += a x ; returns y . y (src/cg.jl:240,242)."""
    out = C.c_double()
    _ck(lib().khip_axpy_sqnorm(y.ctx._h, n, a, _p(x), _p(y), C.byref(out)))
    return out.value


def cg_setup_(n, b, x, r, p) -> float:
    """x = 0 ; r = b ; p = b ; returns b . b in one pass (the set-up of cg!, src/cg.jl:153-162 with M = I, no warm start)."""
    out = C.c_double()
    _ck(lib().khip_cg_setup(x.ctx._h, n, _p(b), _p(x), _p(r), _p(p), C.byref(out)))
    return out.value


def cg_update_(n, a, b, r, p, x):
    """x += a p ; p = r + b p in one pass (src/cg.jl:239,259)."""
    _ck(lib().khip_cg_update(x.ctx._h, n, a, b, _p(r), _p(p), _p(x)))
    return p, x


def waxpy_(n, w, x, b, y):
    _ck(lib().khip_waxpy(w.ctx._h, n, _p(w), _p(x), b, _p(y)))
    return w


def dot2(n, x, y):
    out = (C.c_double * 2)()
    _ck(lib().khip_dot2(x.ctx._h, n, _p(x), _p(y), out))
    return out[0], out[1]


def mgs_(n, V, q, accumulate_into=None, want_norm=True):
    k = len(V)
    ptrs = (C.c_void_p * max(k, 1))(*[_p(v) for v in V])
    h = (C.c_double * max(k, 1))()
    if accumulate_into is not None:
        for i in range(k):
            h[i] = accumulate_into[i]
    nrm = C.c_double()
    _ck(lib().khip_mgs(q.ctx._h, n, k, ptrs, _p(q), h, C.byref(nrm) if want_norm else None,
                       1 if accumulate_into is not None else 0))
    return [h[i] for i in range(k)], (nrm.value if want_norm else None)


def multi_axpy_(n, y, V, x):
    k = len(V)
    ptrs = (C.c_void_p * max(k, 1))(*[_p(v) for v in V])
    coef = (C.c_double * max(k, 1))(*[float(c) for c in y])
    _ck(lib().khip_multi_axpy(x.ctx._h, n, k, coef, ptrs, _p(x)))
    return x


def test_multi_dot(n, V, q):
    """TEST-ONLY (khip_test_multi_dot): [V_i . q] through multi_dot4_kernel and the device scalar ring, as gmres! variant = 1 does."""
    k = len(V)
    ptrs = (C.c_void_p * max(k, 1))(*[_p(v) for v in V])
    out = (C.c_double * max(k, 1))()
    _ck(lib().khip_test_multi_dot(q.ctx._h, n, k, ptrs, _p(q), out))
    return [out[i] for i in range(k)]


def test_multi_axpy_dev_(n, coef, V, x):
    """TEST-ONLY (khip_test_multi_axpy_dev): x <- x - sum_j coef[j] V_j with the coefficients read from the device scalar ring."""
    k = len(V)
    ptrs = (C.c_void_p * max(k, 1))(*[_p(v) for v in V])
    c = (C.c_double * max(k, 1))(*[float(t) for t in coef])
    _ck(lib().khip_test_multi_axpy_dev(x.ctx._h, n, k, c, ptrs, _p(x)))
    return x


def test_divcopy_dev_(n, sumsq, x, y):
    """TEST-ONLY (khip_test_divcopy_dev): y = x / sqrt(sumsq), sumsq read from the device scalar ring (gmres! look-ahead)."""
    _ck(lib().khip_test_divcopy_dev(x.ctx._h, n, float(sumsq), _p(x), _p(y)))
    return y


test_multi_dot.__test__ = test_multi_axpy_dev_.__test__ = test_divcopy_dev_.__test__ = False     # not pytest items


# --------------------------------------------------------------------------- CSR operator

class CsrMatrix:
    """CSR operator resident in HBM; `size`, `eltype`, `kmul_` = the operator contract
    (docs/src/matrix_free.md:32-34)."""

    eltype = np.float64

    def __init__(self, ctx: Context, handle, keep=None):
        self.ctx, self._h, self._keep = ctx, handle, keep
        m, n, nnz = C.c_int64(), C.c_int64(), C.c_int64()
        _ck(lib().khip_csr_shape(handle, C.byref(m), C.byref(n), C.byref(nnz)))
        self.m, self.n, self.nnz = m.value, n.value, nnz.value

    @property
    def shape(self):
        return (self.m, self.n)

    @property
    def spmv_bytes(self) -> int:
        b = C.c_int64()
        _ck(lib().khip_spmv_bytes(self._h, C.byref(b)))
        return b.value

    @property
    def spmv_bytes_stored(self) -> int:
        b = C.c_int64()
        _ck(lib().khip_spmv_bytes_stored(self._h, C.byref(b)))
        return b.value

    @property
    def code_info(self):
        """(bits, diagonals) of the column stream the staged SpMV reads: (32, 0) = plain int32 columns, (8 | 16, T) =
        dictionary-coded diagonals (csrc/colcode.hip), built by the first product that can use it."""
        b, t = C.c_int(), C.c_int()
        _ck(lib().khip_csr_code_info(self._h, C.byref(b), C.byref(t)))
        return b.value, t.value

    @property
    def sell_info(self):
        """(state, units_per_slice, total_units) of the sliced form of a coded operator (khip_csr_sell_info, csrc/colcode.hip
        csr_build_sell): state 1 = built and read by spmv_sell_kernel, 0 = not tried, -1 = not usable."""
        st, u, t = C.c_int(), C.c_int(), C.c_int64()
        _ck(lib().khip_csr_sell_info(self._h, C.byref(st), C.byref(u), C.byref(t)))
        return st.value, u.value, t.value

    @property
    def sell_narrow(self) -> bool:
        """True when the sliced form keeps eight 4-bit codes per row in one 32-bit word (khip_csr_sell_narrow)."""
        v = C.c_int()
        _ck(lib().khip_csr_sell_narrow(self._h, C.byref(v)))
        return bool(v.value)

    @property
    def sell_entries(self) -> int:
        """Pairs (column - row, value bits) in the dictionary of an entry-coded sliced copy (khip_csr_sell_entries); 0 when the
        copy is not entry-coded."""
        v = C.c_int()
        _ck(lib().khip_csr_sell_entries(self._h, C.byref(v)))
        return v.value

    @property
    def sell32_info(self):
        """(state, units_per_slice, total_units) of the sliced form with int32 columns (khip_csr_sell32_info)."""
        st, u, t = C.c_int(), C.c_int(), C.c_int64()
        _ck(lib().khip_csr_sell32_info(self._h, C.byref(st), C.byref(u), C.byref(t)))
        return st.value, u.value, t.value

    @property
    def spmv_kernel_choice(self):
        """The SpMV kernel this handle takes under the context's current options (khip_spmv_kernel_info): 1 stream, 2 vector,
        3 ordered, 4 staged rows, 5 row templates, 6 wave-private windows."""
        k = C.c_int()
        _ck(lib().khip_spmv_kernel_info(self.ctx._h, self._h, C.byref(k)))
        return k.value

    @property
    def delta_info(self):
        """(bits, rows_per_block, escapes) of the block-delta column stream the stream SpMV reads (csrc/coldelta.hip):
        (32, 0, 0) = plain int32 columns."""
        b, r, e = C.c_int(), C.c_int(), C.c_int64()
        _ck(lib().khip_csr_delta_info(self._h, C.byref(b), C.byref(r), C.byref(e)))
        return b.value, r.value, e.value

    @property
    def tile_info(self):
        """dict(state, window, grid_tiles, groups, direct_groups, reuse): the p = 16 SpMM kernel of this handle
        (csrc/spmm_tile.hip); state 1 = wave-private LDS windows, -1 = not usable, 0 = no 16-column product yet."""
        st, w, gt = C.c_int(), C.c_int(), C.c_int()
        g, d, r = C.c_int64(), C.c_int64(), C.c_double()
        _ck(lib().khip_csr_tile_info(self._h, C.byref(st), C.byref(w), C.byref(gt), C.byref(g), C.byref(d), C.byref(r)))
        return dict(state=st.value, window=w.value, grid_tiles=gt.value, groups=g.value, direct_groups=d.value, reuse=r.value)

    TILE_RECORD_FIELDS = ("state", "cap", "stride", "groups", "run_len", "runs", "ahead", "grid_tiles", "direct", "line_rows",
                          "plane_rows", "m", "n", "nnz", "n_ghost", "band")

    def tile_records(self) -> dict:
        """TEST-ONLY (khip_test_csr_tile_records): the build outcome of the tile SpMM, the raw group records ("meta": uint8
        [groups, stride]) and the list of the groups on the direct path ("direct_list")."""
        out, reuse = (_i64 * 16)(), C.c_double()
        _ck(lib().khip_test_csr_tile_records(self._h, out, C.byref(reuse), None, 0, None, 0))
        d = {k: int(out[i]) for i, k in enumerate(self.TILE_RECORD_FIELDS)}
        d["reuse"] = reuse.value
        meta = np.zeros((d["groups"], d["stride"]), dtype=np.uint8)
        dl = np.zeros(d["direct"], dtype=np.int32)
        if d["state"] == 1:
            _ck(lib().khip_test_csr_tile_records(self._h, out, C.byref(reuse), meta.ctypes.data, meta.size,
                                                 dl.ctypes.data_as(C.POINTER(C.c_int32)), dl.size))
        d["meta"], d["direct_list"] = meta, dl
        return d

    @property
    def window_info(self):
        """TEST-ONLY (khip_test_csr_window_info): (win_L, groups, flagged groups) of the window SpMM's metadata."""
        wl, g, f = C.c_int(), _i64(), _i64()
        _ck(lib().khip_test_csr_window_info(self._h, C.byref(wl), C.byref(g), C.byref(f)))
        return wl.value, g.value, f.value

    @property
    def halo_info(self):
        """(gather_mode, n_ghost, n_send) of a distributed handle: how the remote part of x is fetched before a product."""
        g, ng, ns = C.c_int(), C.c_int64(), C.c_int64()
        _ck(lib().khip_csr_halo_info(self._h, C.byref(g), C.byref(ng), C.byref(ns)))
        return g.value, ng.value, ns.value

    def transpose(self) -> "CsrMatrix":
        """A' as its own handle: `At.matvec(x, y)` is `mul!(y, A', x)` (docs/src/matrix_free.md:36-42)."""
        h = C.c_void_p()
        _ck(lib().khip_csr_transpose(self.ctx._h, self._h, C.byref(h)))
        return CsrMatrix(self.ctx, h)

    def to_host_arrays(self):
        """(rowptr, col, val) as the handle holds them, copied to the host (test export khip_test_csr_arrays)."""
        rp = np.empty(self.m + 1, dtype=np.int32)
        cl = np.empty(self.nnz, dtype=np.int32)
        vl = np.empty(self.nnz, dtype=np.float64)
        _ck(lib().khip_test_csr_arrays(self._h, rp.ctypes.data_as(C.POINTER(C.c_int32)), cl.ctypes.data_as(C.POINTER(C.c_int32)),
                                       vl.ctypes.data_as(c_double_p)))
        return rp, cl, vl

    def compress(self) -> int:
        """Re-encode as row templates when the operator repeats few (column - row, value) rows (stencils);
        returns the number of templates, 0 if it stays CSR.  SpMV results are bit-identical either way."""
        t = C.c_int()
        _ck(lib().khip_csr_compress(self.ctx._h, self._h, C.byref(t)))
        return t.value

    @classmethod
    def from_host(cls, ctx, rowptr, col, val, shape, index_base=0, dist_rows=None, n_global=None):
        rowptr = np.ascontiguousarray(rowptr)
        bits = 64 if rowptr.dtype == np.int64 else 32
        if bits == 32:
            rowptr = rowptr.astype(np.int32, copy=False)
        col = np.ascontiguousarray(col, dtype=np.int32)
        val = np.ascontiguousarray(val, dtype=np.float64)
        h = C.c_void_p()
        if dist_rows is None:
            _ck(lib().khip_csr_create(ctx._h, shape[0], shape[1], val.size, rowptr.ctypes.data, bits, col.ctypes.data,
                                      val.ctypes.data, index_base, 0, C.byref(h)))
        else:
            _ck(lib().khip_csr_create_dist(ctx._h, n_global, dist_rows[0], dist_rows[1] - dist_rows[0], val.size,
                                           rowptr.ctypes.data, bits, col.ctypes.data, val.ctypes.data, index_base, 0,
                                           C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def from_scipy(cls, ctx, S):
        S = S.tocsr()
        S.sort_indices()
        return cls.from_host(ctx, S.indptr, S.indices, S.data, S.shape)

    @classmethod
    def banded_random(cls, ctx, n, half_band=13, links=3, seed=1, unsym=False, dense_rows=0, rows=None, distributed=False):
        """The "banded + random, fixed seed" benchmark operator (csrc/gen_irregular.cpp): the non-stencil stand-in for the
        SuiteSparse matrices of benchmark/cg_bmark.jl:29-54 -- a thinned symmetric band plus seeded long-range links,
        diagonally dominant; unsym halves the entries above the diagonal, dense_rows adds rows of 3000 more entries."""
        r0, r1 = rows if rows is not None else (0, n)
        rp, cl, vl, nnz = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int64()
        _ck(lib().khip_gen_banded_random(ctx._h, n, half_band, links, seed, 1 if unsym else 0, dense_rows, r0, r1 - r0,
                                         C.byref(rp), C.byref(cl), C.byref(vl), C.byref(nnz)))
        h = C.c_void_p()
        try:
            if distributed:
                _ck(lib().khip_csr_create_dist(ctx._h, n, r0, r1 - r0, nnz.value, rp, 32, cl, vl, 0, 1, C.byref(h)))
            else:
                if (r0, r1) != (0, n):
                    raise ValueError("a row slice needs distributed=True")
                _ck(lib().khip_csr_create(ctx._h, n, n, nnz.value, rp, 32, cl, vl, 0, 1, C.byref(h)))
        finally:
            for p in (rp, cl, vl):
                lib().khip_free(ctx._h, p)
        return cls(ctx, h)

    @classmethod
    def stencil(cls, ctx, kind: str, n1, n2=None, n3=None, rows=None, distributed=False):
        """Device-side generator of the benchmark operators: 'poisson' = get_div_grad(n1,n2,n3)
        (test/get_div_grad.jl:8-25), 'kron_unsymmetric' (test/test_utils.jl:160-169), 'stencil27' (cfg 5)."""
        kinds = {"poisson": 0, "kron_unsymmetric": 1, "stencil27": 2}
        n2 = n2 or n1
        n3 = n3 or n1
        n = n1 * n2 * n3
        r0, r1 = rows if rows is not None else (0, n)
        rp, cl, vl, nnz = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int64()
        _ck(lib().khip_gen_stencil(ctx._h, kinds[kind], n1, n2, n3, r0, r1 - r0, C.byref(rp), C.byref(cl),
                                   C.byref(vl), C.byref(nnz)))
        h = C.c_void_p()
        try:
            if distributed:
                _ck(lib().khip_csr_create_dist(ctx._h, n, r0, r1 - r0, nnz.value, rp, 32, cl, vl, 0, 1, C.byref(h)))
            else:
                if (r0, r1) != (0, n):
                    raise ValueError("a row slice needs distributed=True")
                _ck(lib().khip_csr_create(ctx._h, n, n, nnz.value, rp, 32, cl, vl, 0, 1, C.byref(h)))
        finally:
            for p in (rp, cl, vl):
                lib().khip_free(ctx._h, p)
        return cls(ctx, h)

    def __del__(self):
        try:
            if self._h and self.ctx._h:
                lib().khip_csr_destroy(self._h)
        except Exception:
            pass

    def diagonal(self) -> DeviceVector:
        d = DeviceVector(self.ctx, self.m)
        _ck(lib().khip_csr_diagonal(self.ctx._h, self._h, d.ptr))
        return d

    def matvec(self, x: DeviceVector, y: DeviceVector | None = None) -> DeviceVector:
        y = y if y is not None else DeviceVector(self.ctx, self.m)
        return kmul_(y, self, x)


def gen_stencil_arrays(ctx, kind, n1, n2=None, n3=None, rows=None):
    """Raw (rowptr, col, val) of the device generator copied to host -- used by the parity tests."""
    kinds = {"poisson": 0, "kron_unsymmetric": 1, "stencil27": 2}
    n2 = n2 or n1
    n3 = n3 or n1
    n = n1 * n2 * n3
    r0, r1 = rows if rows is not None else (0, n)
    rp, cl, vl, nnz = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int64()
    _ck(lib().khip_gen_stencil(ctx._h, kinds[kind], n1, n2, n3, r0, r1 - r0, C.byref(rp), C.byref(cl), C.byref(vl),
                               C.byref(nnz)))
    m = r1 - r0
    rowptr = np.empty(m + 1, dtype=np.int32)
    col = np.empty(nnz.value, dtype=np.int32)
    val = np.empty(nnz.value, dtype=np.float64)
    _ck(lib().khip_memcpy_d2h(ctx._h, rowptr.ctypes.data, rp, 4 * (m + 1)))
    if nnz.value:
        _ck(lib().khip_memcpy_d2h(ctx._h, col.ctypes.data, cl, 4 * nnz.value))
        _ck(lib().khip_memcpy_d2h(ctx._h, val.ctypes.data, vl, 8 * nnz.value))
    for p in (rp, cl, vl):
        lib().khip_free(ctx._h, p)
    return rowptr, col, val


def gen_banded_random_arrays(ctx, n, half_band=13, links=3, seed=1, unsym=False, dense_rows=0, rows=None):
    """Raw (rowptr, col, val) of khip_gen_banded_random copied to host -- used by the parity tests."""
    r0, r1 = rows if rows is not None else (0, n)
    rp, cl, vl, nnz = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int64()
    _ck(lib().khip_gen_banded_random(ctx._h, n, half_band, links, seed, 1 if unsym else 0, dense_rows, r0, r1 - r0,
                                     C.byref(rp), C.byref(cl), C.byref(vl), C.byref(nnz)))
    m = r1 - r0
    rowptr = np.empty(m + 1, dtype=np.int32)
    col = np.empty(nnz.value, dtype=np.int32)
    val = np.empty(nnz.value, dtype=np.float64)
    _ck(lib().khip_memcpy_d2h(ctx._h, rowptr.ctypes.data, rp, 4 * (m + 1)))
    if nnz.value:
        _ck(lib().khip_memcpy_d2h(ctx._h, col.ctypes.data, cl, 4 * nnz.value))
        _ck(lib().khip_memcpy_d2h(ctx._h, val.ctypes.data, vl, 8 * nnz.value))
    for p in (rp, cl, vl):
        lib().khip_free(ctx._h, p)
    return rowptr, col, val


# --------------------------------------------------------------------------- solvers

class SimpleStats:
    """SimpleStats (src/krylov_stats.jl:24-44)."""

    def __init__(self, st: CStats):
        self.niter = st.niter
        self.solved = bool(st.solved)
        self.inconsistent = bool(st.inconsistent)
        self.indefinite = bool(st.indefinite)
        self.npcCount = st.npcCount
        self.timer = st.timer
        self.allocation_timer = st.allocation_timer
        self.status = st.status.decode("utf-8")
        self.residuals = np.array([st.residuals[i] for i in range(st.nres)]) if st.nres else np.zeros(0)
        self.error = st.error.decode("utf-8")

    def __repr__(self):
        return f"SimpleStats(niter={self.niter}, solved={self.solved}, status={self.status!r})"


class AdjointStats:
    """AdjointStats (src/krylov_stats.jl): one history and one flag per system; `status` is the reference's full string, which
    khip_stats.status cannot always hold (khip_bilqr_adjoint_stats).  `solved` and `residuals` are the C struct's summary: both
    sides solved, the primal history."""

    def __init__(self, st: CStats, solved_primal, solved_dual, residuals_primal, residuals_dual, status):
        self.niter = st.niter
        self.solved_primal = bool(solved_primal)
        self.solved_dual = bool(solved_dual)
        self.solved = bool(st.solved)
        self.inconsistent = bool(st.inconsistent)         # trilqr!: the dual side's flag (always False for bilqr!)
        self.residuals_primal = residuals_primal
        self.residuals_dual = residuals_dual
        self.residuals = residuals_primal
        self.timer = st.timer
        self.allocation_timer = st.allocation_timer
        self.status = status
        self.error = st.error.decode("utf-8")

    def __repr__(self):
        return (f"AdjointStats(niter={self.niter}, solved_primal={self.solved_primal}, solved_dual={self.solved_dual}, "
                f"status={self.status!r})")


_ILU_PATH_FIELDS = ("fast", "wide", "packed", "packed_pad0", "long_row_blocks", "long_face_blocks", "max_faces", "max_row",
                    "max_levels", "max_width", "rows_cap", "lds", "workgroups", "blocks")


def _ilu_paths_dict(out):
    """paths48 of khip_test_ilu0_paths / khip_test_ilu_paths_host (include/krylov_hip_test.h) as a dict."""
    tri = lambda o: {k: int(out[o + i]) for i, k in enumerate(_ILU_PATH_FIELDS)}
    lev = lambda o: {"batched": int(out[o]), "single": int(out[o + 1])}
    return {"lower": tri(0), "upper": tri(16), "levels": {"factor": lev(32), "lower": lev(34), "upper": lev(36)},
            "blocks_in_use": int(out[38]), "fallback": int(out[39]), "attempted": int(out[40]), "nlevels": (int(out[41]), int(out[42]))}


def ilu_paths_host(rowptr, col, ilu_blocks=1, mode=1):
    """Test-only, no device: what Ilu0.path_info() would report for an operator with this CSR pattern created under option
    ilu_blocks (workgroups = 0: it depends on the device), plus the fields of khip_test_ilu_blocks_host under "analysis"."""
    rp = np.ascontiguousarray(rowptr, dtype=np.int64)
    ci = np.ascontiguousarray(col, dtype=np.int32)
    out10, out48 = (_i64 * 10)(), (_i64 * 48)()
    _ck(lib().khip_test_ilu_paths_host(len(rp) - 1, rp.ctypes.data_as(C.POINTER(_i64)), ci.ctypes.data_as(C.POINTER(C.c_int32)), mode,
                                       ilu_blocks, out10, out48))
    d = _ilu_paths_dict(out48)
    d["analysis"] = dict(dims=tuple(out10[0:3]), skew=out10[3], nb=(out10[4], out10[5]), max_ext=out10[6], rec_ok=out10[7],
                         max_row=out10[8], rows_cap=out10[9])
    return d


class Ilu0:
    """ILU(0) of A on its own pattern as the operator y = U \\ (L \\ x); for SPD A this is IC(0).  Usable as the
    M / N argument of cg_ / gmres_ / bicgstab_ (the reference's ic02 / ilu02 recipes, docs/src/gpu.md:74-163)."""

    def __init__(self, A: "CsrMatrix", graph: bool = True):
        self.ctx, self.n, self.A = A.ctx, A.m, A
        self.op = COperator()
        _ck(lib().khip_ilu0_create(A.ctx._h, A._h, C.byref(self.op)))
        if not graph:
            _ck(lib().khip_ilu0_set_graph(C.byref(self.op), 0))

    def __call__(self, x, y):
        rc = self.op.apply(self.op.self, _p(x), _p(y))
        if rc:
            raise KhipError(rc, lib().khip_last_error().decode())
        return y

    @property
    def levels(self):
        lo, up = _i64(), _i64()
        _ck(lib().khip_ilu0_info(C.byref(self.op), C.byref(lo), C.byref(up), None))
        return lo.value, up.value

    def block_info(self):
        """(grid dims the pattern was recognised as, or (0, 0, 0); blocks per triangle -- 0: level scheduling, > 0 with dims
        (0, 0, 0): blocks from the level-sorted row sequence; 1 if a bounded spin of the block schedule ever gave up).
        Synchronises."""
        dims, nb, failed = (_i64 * 3)(), _i64(), _int()
        _ck(lib().khip_ilu0_block_info(C.byref(self.op), dims, C.byref(nb), C.byref(failed)))
        return tuple(dims), nb.value, failed.value

    def path_info(self):
        """Test-only: which row path the blocks of the two block solves take ("lower" / "upper": blocks on the fast, wide and
        packed path, packed ones inside a handle with records, blocks with rows > 16 entries or > 1024 face rows, the largest
        face list / row / local level count / local level, rows_cap, LDS bytes, workgroups launched, blocks) and how the level
        schedule is launched ("levels": batched small-level launches and single-level launches per kind)."""
        out = (_i64 * 48)()
        _ck(lib().khip_test_ilu0_paths(C.byref(self.op), out))
        return _ilu_paths_dict(out)

    def values(self):
        """Factor values on A's pattern (host copy)."""
        p = C.c_void_p()
        _ck(lib().khip_ilu0_info(C.byref(self.op), None, None, C.byref(p)))
        return DeviceVector(self.ctx, self.A.nnz, ptr=p.value, owner=self).to_host()

    def __del__(self):
        try:
            if self.ctx._h:
                lib().khip_ilu0_destroy(C.byref(self.op))
        except Exception:
            pass


def _make_operator(ctx, op, n, keep):
    """CsrMatrix | callable(x: DeviceVector, y: DeviceVector) | None -> POINTER(COperator) or None."""
    if op is None:
        return None
    if isinstance(op, (Jacobi, Ilu0)):  # native operator: no Python in the loop
        keep.append(op)
        return C.byref(op.op)
    co = COperator()
    if isinstance(op, CsrMatrix):
        co.csr = op._h
        co.apply = C.cast(None, APPLY_FN)
    else:
        def thunk(_self, xp, yp):
            try:
                op(DeviceVector(ctx, n, ptr=xp), DeviceVector(ctx, n, ptr=yp))
                return 0
            except Exception as e:  # never propagate across the C boundary
                sys.stderr.write(f"operator callback failed: {e}\n")
                return 1
        fn = APPLY_FN(thunk)
        keep.append(fn)
        co.csr = None
        co.apply = fn
    keep.append(co)
    return C.byref(co)


# The reference's entry points forward EVERY keyword to the in-place method explicitly, their own defaults included:
# `cg(A, b)`, `krylov_solve(Val(:cg), A, b)`, `krylov_solve!(ws, A, b)` and the x0 forms all call
# `cg!(ws, A, b; M, ldiv, ..., callback, iostream)` with `callback = workspace -> false` (src/cg.jl:110, src/interface.jl:146-154,
# 266-275, 331, 336-345).  A binding that takes its device-resident loop only when NO callback was passed would therefore never take
# it from those entry points: the default callback has to be recognised for what it is.  `default_callback` below is
# this mirror's `workspace -> false`; `_user_callback` maps it (and None) to "no callback", exactly as `user_callback` in
# julia/KrylovHIP/src/KrylovHIP.jl maps the anonymous functions the reference's generated methods forward.
def default_callback(workspace) -> bool:          # `callback = workspace -> false`
    return False


def _user_callback(callback):
    return None if (callback is None or callback is default_callback) else callback


def _log_fd(iostream) -> int:
    """The reference's `iostream` keyword (default kstdout) as khip_options.log_fd: 0 = stdout, else the caller's descriptor."""
    if iostream is None or iostream is sys.stdout:
        return 0
    if isinstance(iostream, int):
        return iostream
    iostream.flush()
    return iostream.fileno()


def _make_options(atol=None, rtol=None, itmax=0, timemax=None, history=False, radius=0.0, linesearch=False,
                  restart=False, reorthogonalization=False, fused=True, callback=None, keep=None, ws=None, variant=0, verbose=0, log_fd=0,
                  ldiv=False, iostream=None):
    if ldiv:        # `ldiv = true` applies M / N with ldiv! (src/krylov_utils.jl:307): a factorisation object of the HOST language
        raise KhipError(-4, "ldiv = true has no meaning across the C ABI: pass M / N as operators z <- M r (Jacobi, Ilu0, a callable)")
    if iostream is not None:
        log_fd = _log_fd(iostream)
    if timemax is not None:
        # Inf (the reference's default) = no limit = the C default; a limit the entry point has already used up
        # (`timemax -= elapsed_time`, src/interface.jl:151) stays a limit: the C side reads <= 0 as "none"
        timemax = None if math.isinf(timemax) else max(timemax, sys.float_info.min)
    callback = _user_callback(callback)
    o = lib().khip_default_options()
    if atol is not None:
        o.atol = atol
    if rtol is not None:
        o.rtol = rtol
    o.itmax = int(itmax)
    if timemax is not None:
        o.timemax = timemax
    o.history = int(history)
    o.radius = radius
    o.linesearch = int(linesearch)
    o.restart = int(restart)
    o.reorthogonalization = int(reorthogonalization)
    o.fused = 2 if fused is True else int(fused)     # True = everything that is bit-identical: fused kernels + device-resident scalars
    o.variant = int(variant)
    o.verbose = int(verbose)
    o.log_fd = int(log_fd)          # the reference's `iostream`: 0 = stdout, else a file descriptor
    if callback is not None:
        def cb(_ws, _ud):
            try:
                return 1 if callback(ws) else 0
            except Exception as e:
                sys.stderr.write(f"callback failed: {e}\n")
                return 1
        fn = CALLBACK_FN(cb)
        keep.append(fn)
        o.callback = fn
    return o


# Workspaces own their vectors on THIS side, as the reference's do on the Julia side (`x, r, p, Ap :: S`,
# src/krylov_workspaces.jl:236-291), and hand the device pointers to the library (khip_*_workspace_adopt): the solvers run on the
# caller's vectors, `solution(ws) is ws.x`.  This is the executed twin of julia/KrylovHIP/src/KrylovHIP.jl.  `adopt=False` (or
# KHIP_PY_WORKSPACES=create in the environment) takes the library-owned workspaces of khip_*_workspace_create instead.
def _adopt_default() -> bool:
    return os.environ.get("KHIP_PY_WORKSPACES", "adopt") != "create"


class _Workspace:
    _prefix = ""
    _fields = ()

    def _fn(self, name):
        return getattr(lib(), f"khip_{self._prefix}_{name}")

    def __del__(self):
        try:
            if self._h and self.ctx._h:
                self._fn("workspace_destroy")(self._h)
        except Exception:
            pass

    def _adopt_vector(self, name: str, v: "DeviceVector"):
        """allocate_if(..., workspace, :name, S, workspace.x) followed by the hand-over of the pointer."""
        self._vec[name] = v
        _ck(self._fn("workspace_adopt_vector")(self._h, name.encode(), v.ptr))
        return v

    def _len(self, name: str) -> int:
        """Entries of the vector `name`: n, but for the row side of a _TwoSidedWorkspace."""
        return self.n

    def _allocate_if(self, cond: bool, name: str):
        """src/krylov_utils.jl:281-288: allocate the lazily-held vector `name` on first need."""
        if cond and self.adopted and name not in self._vec:
            t0 = time.perf_counter()
            v = self.ctx.empty(self._len(name))
            self._alloc_s += time.perf_counter() - t0            # stats.allocation_timer counts the lazy allocations too
            self._adopt_vector(name, v)

    @property
    def x(self) -> DeviceVector:
        """solution(workspace) === workspace.x (src/workspace_accessors.jl:151, test/test_interface.jl:260)."""
        if self.adopted:
            return self._vec["x"]
        return DeviceVector(self.ctx, self.n, ptr=self._fn("solution")(self._h), owner=self)

    @property
    def stats(self) -> SimpleStats:
        st = SimpleStats(self._fn("stats")(self._h).contents)
        if self.adopted:                                  # the vectors were allocated (and timed) on this side
            st.allocation_timer += self._alloc_s
        st.timer += getattr(self, "_timer_extra", 0.0)    # `workspace.stats.timer += elapsed_time`, src/interface.jl:153
        return st

    @property
    def last_path(self) -> int:
        """Which loop the last solve ran (khip_*_last_path): 2 device-resident / look-ahead, 1 host-driven fused, 0 one launch per
        primitive, -1 none yet.  What KrylovHIP.NATIVE_SOLVES / LAST_PATH report on the Julia side."""
        return self._fn("last_path")(self._h)

    def warm_start_(self, x0: DeviceVector):
        """warm_start!(workspace, x0) (src/workspace_accessors.jl:193-200): allocate_if(true, ws, :Δx, ...); kcopy!(n, ws.Δx, x0)."""
        if self.adopted:
            self._allocate_if(True, "dx")
            kcopy_(self.n, self._vec["dx"], x0)
            _ck(self._fn("warm_start")(self._h, self._vec["dx"].ptr))     # same pointer: only sets the flag
        else:
            _ck(self._fn("warm_start")(self._h, _p(x0)))
        return self

    @property
    def nbytes(self) -> int:
        return self._fn("workspace_bytes")(self._h)


class CgWorkspace(_Workspace):
    """CgWorkspace(m, n, S) (src/krylov_workspaces.jl:236-291)."""
    _prefix = "cg"

    def __init__(self, ctx: Context, m: int, n: int, adopt: bool | None = None):
        self.ctx, self.m, self.n = ctx, m, n
        self.adopted = _adopt_default() if adopt is None else bool(adopt)
        self._h = C.c_void_p()
        if self.adopted:
            t0 = time.perf_counter()
            self._vec = {k: ctx.empty(n) for k in ("x", "r", "p", "Ap")}     # S(undef, n) x 4; dx, npc_dir, z stay empty
            self._alloc_s = time.perf_counter() - t0
            v = self._vec
            _ck(lib().khip_cg_workspace_adopt(ctx._h, m, n, v["x"].ptr, v["r"].ptr, v["p"].ptr, v["Ap"].ptr, C.byref(self._h)))
        else:
            _ck(lib().khip_cg_workspace_create(ctx._h, m, n, C.byref(self._h)))

    def vector(self, name: str):
        if self.adopted and name in self._vec:
            return self._vec[name]
        p = lib().khip_cg_vector(self._h, name.encode())
        return DeviceVector(self.ctx, self.n, ptr=p, owner=self) if p else None


class GmresWorkspace(_Workspace):
    """GmresWorkspace(m, n, S; memory = 20) (src/krylov_workspaces.jl:2857-2924)."""
    _prefix = "gmres"

    def __init__(self, ctx: Context, m: int, n: int, memory: int = 20, adopt: bool | None = None):
        self.ctx, self.m, self.n, self.memory = ctx, m, n, memory
        self.adopted = _adopt_default() if adopt is None else bool(adopt)
        self._h = C.c_void_p()
        if self.adopted:
            mem = 20 if memory <= 0 else memory
            mem = min(m, mem)                                                  # memory = min(m, memory), :2900
            t0 = time.perf_counter()
            self._vec = {k: ctx.empty(n) for k in ("x", "w")}
            self.V = [ctx.empty(n) for _ in range(mem)]                        # V = S[S(undef, n) for i = 1 : memory]
            self._alloc_s = time.perf_counter() - t0
            ptrs = (C.c_void_p * max(mem, 1))(*[v.ptr for v in self.V])
            _ck(lib().khip_gmres_workspace_adopt(ctx._h, m, n, mem, self._vec["x"].ptr, self._vec["w"].ptr, ptrs, C.byref(self._h)))

            def grow(_ud):                                                     # push!(V, similar(x)), src/gmres.jl:319-324
                try:
                    self.V.append(self.ctx.empty(self.n))
                    return self.V[-1].ptr
                except Exception as e:
                    sys.stderr.write(f"grow callback failed: {e}\n")
                    return None
            self._grow = GROW_FN(grow)
            _ck(lib().khip_gmres_workspace_set_grow(self._h, self._grow, None))
        else:
            _ck(lib().khip_gmres_workspace_create(ctx._h, m, n, memory, C.byref(self._h)))

    def host_state(self):
        """(c, s, z, R, inner_iter) of the last solve: the host fields of the reference's workspace (:2866-2871)."""
        ln, it = C.c_int(), C.c_int()
        _ck(lib().khip_gmres_host_state(self._h, 0, None, None, None, None, C.byref(ln), C.byref(it)))
        k = ln.value
        c, s_, z, R = np.zeros(k), np.zeros(k), np.zeros(k), np.zeros(k * (k + 1) // 2)
        _ck(lib().khip_gmres_host_state(self._h, k, c.ctypes.data_as(c_double_p), s_.ctypes.data_as(c_double_p),
                                        z.ctypes.data_as(c_double_p), R.ctypes.data_as(c_double_p), C.byref(ln), C.byref(it)))
        return c, s_, z, R, it.value


class BicgstabWorkspace(_Workspace):
    """BicgstabWorkspace(m, n, S) (src/krylov_workspaces.jl:1568-1629)."""
    _prefix = "bicgstab"

    def __init__(self, ctx: Context, m: int, n: int, adopt: bool | None = None):
        self.ctx, self.m, self.n = ctx, m, n
        self.adopted = _adopt_default() if adopt is None else bool(adopt)
        self._h = C.c_void_p()
        if self.adopted:
            t0 = time.perf_counter()
            self._vec = {k: ctx.empty(n) for k in ("x", "r", "p", "v", "s", "qd")}
            self._alloc_s = time.perf_counter() - t0
            v = self._vec
            _ck(lib().khip_bicgstab_workspace_adopt(ctx._h, m, n, v["x"].ptr, v["r"].ptr, v["p"].ptr, v["v"].ptr, v["s"].ptr,
                                                    v["qd"].ptr, C.byref(self._h)))
        else:
            _ck(lib().khip_bicgstab_workspace_create(ctx._h, m, n, C.byref(self._h)))


class MinresWorkspace(_Workspace):
    """MinresWorkspace(m, n, S; window = 5) (src/krylov_workspaces.jl:77-114).  stats carries Aresiduals and Acond."""
    _prefix = "minres"

    def __init__(self, ctx: Context, m: int, n: int, window: int = 5, adopt: bool | None = None):
        self.ctx, self.m, self.n, self.window = ctx, m, n, window
        self.adopted = _adopt_default() if adopt is None else bool(adopt)
        self._h = C.c_void_p()
        if self.adopted:
            t0 = time.perf_counter()
            self._vec = {k: ctx.empty(n) for k in ("x", "r1", "r2", "w1", "w2", "y")}     # dx, npc_dir, v stay empty
            self._alloc_s = time.perf_counter() - t0
            v = self._vec
            _ck(lib().khip_minres_workspace_adopt(ctx._h, m, n, window, v["x"].ptr, v["r1"].ptr, v["r2"].ptr, v["w1"].ptr,
                                                  v["w2"].ptr, v["y"].ptr, C.byref(self._h)))
        else:
            _ck(lib().khip_minres_workspace_create(ctx._h, m, n, window, C.byref(self._h)))

    @property
    def stats(self) -> SimpleStats:
        st = super().stats
        ar, nar, ac, nac = c_double_p(), _int(), c_double_p(), _int()
        _ck(lib().khip_minres_histories(self._h, C.byref(ar), C.byref(nar), C.byref(ac), C.byref(nac)))
        st.Aresiduals = np.array(ar[:nar.value]) if nar.value else np.zeros(0)
        st.Acond = np.array(ac[:nac.value]) if nac.value else np.zeros(0)
        return st

    @property
    def fused_product(self) -> bool:
        """The last solve's Lanczos step ran inside the sliced SpMV (khip_minres_fused_product)."""
        return lib().khip_minres_fused_product(self._h) == 1

    def vector(self, name: str):
        if self.adopted and name in self._vec:
            return self._vec[name]
        p = lib().khip_minres_vector(self._h, name.encode())
        return DeviceVector(self.ctx, self.n, ptr=p, owner=self) if p else None


class LanczosShiftStats:
    """LanczosShiftStats (src/krylov_stats.jl): residuals and indefinite per shift."""

    def __init__(self, st: CStats, residuals, indefinite):
        self.niter = st.niter
        self.solved = bool(st.solved)
        self.residuals = residuals
        self.indefinite = indefinite
        self.timer = st.timer
        self.allocation_timer = st.allocation_timer
        self.status = st.status.decode("utf-8")
        self.error = st.error.decode("utf-8")

    def __repr__(self):
        return f"LanczosShiftStats(niter={self.niter}, solved={self.solved}, status={self.status!r})"


class CgLanczosShiftWorkspace(_Workspace):
    """CgLanczosShiftWorkspace(m, n, nshifts, S) (src/krylov_workspaces.jl:616-660): x and p are lists of nshifts DeviceVectors;
    stats.residuals is one history per shift, stats.indefinite one flag per shift."""
    _prefix = "cg_lanczos_shift"
    ARRAYS = ("rNorms", "σ", "δhat", "ω", "γ", "converged", "not_cv", "indefinite")      # khip_cg_lanczos_shift_arrays order

    def __init__(self, ctx: Context, m: int, n: int, nshifts: int, adopt: bool | None = None):
        self.ctx, self.m, self.n, self.nshifts = ctx, m, n, int(nshifts)
        self.adopted = _adopt_default() if adopt is None else bool(adopt)
        self._h = C.c_void_p()
        if self.adopted:
            t0 = time.perf_counter()
            self._vec = {k: ctx.empty(n) for k in ("Mv", "Mv_prev", "Mv_next")}          # v stays empty
            self._x = [ctx.empty(n) for _ in range(self.nshifts)]
            self._pv = [ctx.empty(n) for _ in range(self.nshifts)]
            self._alloc_s = time.perf_counter() - t0
            v = self._vec
            xs = (C.c_void_p * self.nshifts)(*[u.ptr for u in self._x])
            ps = (C.c_void_p * self.nshifts)(*[u.ptr for u in self._pv])
            _ck(lib().khip_cg_lanczos_shift_workspace_adopt(ctx._h, m, n, self.nshifts, v["Mv"].ptr, v["Mv_prev"].ptr,
                                                            v["Mv_next"].ptr, C.cast(xs, c_void_pp), C.cast(ps, c_void_pp),
                                                            C.byref(self._h)))
        else:
            _ck(lib().khip_cg_lanczos_shift_workspace_create(ctx._h, m, n, self.nshifts, C.byref(self._h)))

    def _owned(self, name):
        return DeviceVector(self.ctx, self.n, ptr=lib().khip_cg_lanczos_shift_vector(self._h, name.encode()), owner=self)

    @property
    def x(self):
        """workspace.x: one solution per shift."""
        if self.adopted:
            return list(self._x)
        return [self._owned(f"x{i + 1}") for i in range(self.nshifts)]

    @property
    def p(self):
        if self.adopted:
            return list(self._pv)
        return [self._owned(f"p{i + 1}") for i in range(self.nshifts)]

    def arrays(self) -> dict:
        """The workspace's per-shift host arrays (rNorms, σ, δhat, ω, γ, converged, not_cv) and stats.indefinite."""
        out = np.zeros(8 * self.nshifts)
        _ck(lib().khip_cg_lanczos_shift_arrays(self._h, out.ctypes.data_as(c_double_p)))
        a = {k: out[i * self.nshifts:(i + 1) * self.nshifts].copy() for i, k in enumerate(self.ARRAYS)}
        for k in ("converged", "not_cv", "indefinite"):
            a[k] = a[k] != 0
        return a

    @property
    def rNorms(self):
        return self.arrays()["rNorms"]

    @property
    def converged(self):
        return self.arrays()["converged"]

    @property
    def not_cv(self):
        return self.arrays()["not_cv"]

    @property
    def stats(self) -> LanczosShiftStats:
        res = []
        for i in range(self.nshifts):
            ptr, cnt = c_double_p(), _int()
            _ck(lib().khip_cg_lanczos_shift_residuals(self._h, i, C.byref(ptr), C.byref(cnt)))
            res.append([ptr[j] for j in range(cnt.value)])
        st = LanczosShiftStats(lib().khip_cg_lanczos_shift_stats(self._h).contents, res, list(self.arrays()["indefinite"]))
        if self.adopted:
            st.allocation_timer += self._alloc_s
        st.timer += getattr(self, "_timer_extra", 0.0)
        return st

    def vector(self, name: str):
        if self.adopted and name in self._vec:
            return self._vec[name]
        p = lib().khip_cg_lanczos_shift_vector(self._h, name.encode())
        return DeviceVector(self.ctx, self.n, ptr=p, owner=self) if p else None

    def warm_start_(self, x0):
        raise KhipError(-4, "cg_lanczos_shift! has no warm start")


class _BiLanczosWorkspace(_Workspace):
    """What the workspaces of bilq!, qmr! and bilqr! share: VECTORS come with the workspace (caller-owned: `vectors=` or fresh ones,
    handed to khip_*_workspace_adopt in that order; library-owned with adopt=False), the others stay empty until needed.  The
    fused loops rotate the roles of (vₖ₋₁, vₖ), (uₖ₋₁, uₖ) and of the solver's w vectors, and `vector(name)` follows the role
    (khip_*_vector): after k iterations a name holds what the reference's variable of that name holds."""
    VECTORS = ()
    SOLUTIONS = ("x",)

    def __init__(self, ctx: Context, m: int, n: int, adopt: bool | None = None, vectors=None):
        self.ctx, self.m, self.n = ctx, m, n
        self.adopted = vectors is not None or (_adopt_default() if adopt is None else bool(adopt))
        self._h = C.c_void_p()
        if self.adopted:
            t0 = time.perf_counter()
            self._vec = dict(vectors) if vectors is not None else {k: ctx.empty(n) for k in self.VECTORS}
            self._alloc_s = time.perf_counter() - t0
            _ck(self._fn("workspace_adopt")(ctx._h, m, n, *[self._vec[k].ptr for k in self.VECTORS], C.byref(self._h)))
        else:
            _ck(self._fn("workspace_create")(ctx._h, m, n, C.byref(self._h)))

    def vector(self, name: str):
        if name in self.SOLUTIONS:
            return getattr(self, name)
        p = self._fn("vector")(self._h, name.encode())
        return DeviceVector(self.ctx, self.n, ptr=p, owner=self) if p else None


class BilqWorkspace(_BiLanczosWorkspace):
    """BilqWorkspace(m, n, S) (src/krylov_workspaces.jl): uₖ₋₁, uₖ, q, vₖ₋₁, vₖ, p, x, d̅; Δx, t, s stay empty until needed.  After a
    solve only x and the stats are defined."""
    _prefix = "bilq"
    VECTORS = ("u_prev", "u", "q", "v_prev", "v", "p", "x", "dbar")


class QmrWorkspace(_BiLanczosWorkspace):
    """QmrWorkspace(m, n, S) (src/krylov_workspaces.jl): uₖ₋₁, uₖ, q, vₖ₋₁, vₖ, p, x, wₖ₋₂, wₖ₋₁; Δx, t, s stay empty until needed."""
    _prefix = "qmr"
    VECTORS = ("u_prev", "u", "q", "v_prev", "v", "p", "x", "w_prev2", "w_prev")


class _TwoSidedWorkspace(_Workspace):
    """What the workspaces of the solvers on the Saunders-Simon-Yip process share (usymqr!, usymlq!, trilqr!, tricg!, trimr!, usymlqr!):
    A has m rows and n columns, so a vector has m entries where its name is in ROW_SIDE and n otherwise (`_len`).  VECTORS come with
    the workspace (caller-owned: `vectors=` or fresh ones, handed to khip_*_workspace_adopt in that order; library-owned with
    adopt=False); Δx ("dx") and, with SOLUTIONS == ("x", "y"), Δy ("dy") stay empty until a warm start.  `vector(name)` follows the
    roles the fused loops rotate (khip_*_vector)."""
    VECTORS = ()
    ROW_SIDE = ()
    SOLUTIONS = ("x",)
    ARESIDUALS = False                                    # stats carries the Aresiduals history (khip_*_aresiduals)

    def __init__(self, ctx: Context, m: int, n: int, adopt: bool | None = None, vectors=None):
        self.ctx, self.m, self.n = ctx, m, n
        self.adopted = vectors is not None or (_adopt_default() if adopt is None else bool(adopt))
        self._h = C.c_void_p()
        if self.adopted:
            t0 = time.perf_counter()
            self._vec = dict(vectors) if vectors is not None else {k: ctx.empty(self._len(k)) for k in self.VECTORS}
            self._alloc_s = time.perf_counter() - t0
            _ck(self._fn("workspace_adopt")(ctx._h, m, n, *[self._vec[k].ptr for k in self.VECTORS], C.byref(self._h)))
        else:
            _ck(self._fn("workspace_create")(ctx._h, m, n, C.byref(self._h)))

    def _len(self, name: str) -> int:
        return self.m if name in self.ROW_SIDE else self.n

    def _solution(self, name: str) -> DeviceVector:
        if self.adopted:
            return self._vec[name]
        fn = "solution" if self.SOLUTIONS == ("x",) else "solution_" + name
        return DeviceVector(self.ctx, self._len(name), ptr=self._fn(fn)(self._h), owner=self)

    @property
    def x(self) -> DeviceVector:
        return self._solution("x")

    @property
    def y(self) -> DeviceVector:
        if "y" not in self.SOLUTIONS:
            raise AttributeError("y")
        return self._solution("y")

    @property
    def stats(self) -> SimpleStats:
        st = super().stats
        if self.ARESIDUALS:
            ar, nar = c_double_p(), _int()
            _ck(self._fn("aresiduals")(self._h, C.byref(ar), C.byref(nar)))
            st.Aresiduals = np.array(ar[:nar.value]) if nar.value else np.zeros(0)
        return st

    def vector(self, name: str):
        if name in self.SOLUTIONS:
            return getattr(self, name)
        p = self._fn("vector")(self._h, name.encode())
        return DeviceVector(self.ctx, self._len(name), ptr=p, owner=self) if p else None

    def warm_start_(self, x0: DeviceVector, y0: DeviceVector | None = None):
        """warm_start!(workspace, x0[, y0]) (src/workspace_accessors.jl).  With SOLUTIONS == ("x", "y") both are required, each of
        the length of its Δ: a wrong length is refused before anything is copied."""
        if "y" not in self.SOLUTIONS:
            if y0 is not None:
                raise TypeError(f"{self._prefix}: warm_start_ takes x0 alone")
            return super().warm_start_(x0)
        if y0 is None or x0 is None:
            raise KhipError(-1, f"{self._prefix}: warm_start needs x0 and y0")
        if len(x0) != self._len("dx") or len(y0) != self._len("dy"):
            raise KhipError(-1, "Inconsistent problem size")
        if self.adopted:
            for name, src in (("dx", x0), ("dy", y0)):
                self._allocate_if(True, name)
                kcopy_(self._len(name), self._vec[name], src)
            _ck(self._fn("warm_start")(self._h, self._vec["dx"].ptr, self._vec["dy"].ptr))     # same pointers: only the flag
        else:
            _ck(self._fn("warm_start")(self._h, _p(x0), _p(y0)))
        return self


class UsymqrWorkspace(_TwoSidedWorkspace):
    """UsymqrWorkspace(m, n, Sm, Sn) (src/krylov_workspaces.jl): vₖ₋₁, vₖ, q of m entries and x, wₖ₋₂, wₖ₋₁, uₖ₋₁, uₖ, p of n; Δx ("dx")
    stays empty until a warm start.  stats carries Aresiduals.  The fused loops rotate the roles of (vₖ₋₁, vₖ), (uₖ₋₁, uₖ) and
    (wₖ₋₂, wₖ₋₁), and `vector(name)` follows the role (khip_usymqr_vector): after k iterations a name holds what the reference's
    variable of that name holds.  A rectangular system (m ≠ n) runs the primitive sequence whatever `fused` says: `last_path`
    reports 0."""
    _prefix = "usymqr"
    VECTORS = ("v_prev", "v", "q", "x", "w_prev2", "w_prev", "u_prev", "u", "p")
    ROW_SIDE = ("v_prev", "v", "q")                                             # m entries; every other vector has n
    ARESIDUALS = True


class UsymlqWorkspace(_TwoSidedWorkspace):
    """UsymlqWorkspace(m, n, Sm, Sn) (src/krylov_workspaces.jl): uₖ₋₁, uₖ, p, x, d̅ of n entries and vₖ₋₁, vₖ, q of m; Δx ("dx") stays
    empty until a warm start.  The fused loops rotate the roles of (vₖ₋₁, vₖ) and (uₖ₋₁, uₖ), and `vector(name)` follows the role
    (khip_usymlq_vector): after k iterations a name holds what the reference's variable of that name holds ("dbar" = d̅ₖ).  A
    rectangular system (m ≠ n) runs the primitive sequence whatever `fused` says: `last_path` reports 0."""
    _prefix = "usymlq"
    VECTORS = ("u_prev", "u", "p", "x", "dbar", "v_prev", "v", "q")
    ROW_SIDE = ("v_prev", "v", "q")                                             # m entries; every other vector has n


class TrilqrWorkspace(_TwoSidedWorkspace):
    """TrilqrWorkspace(m, n, Sm, Sn) (src/krylov_workspaces.jl): uₖ₋₁, uₖ, p, d̅, x of n entries and vₖ₋₁, vₖ, q, t ("y"), wₖ₋₃, wₖ₋₂ of m;
    Δx ("dx", n) and Δy ("dy", m) stay empty until a warm start.  stats is an AdjointStats, with `inconsistent` (the dual side's flag)
    beside the reference's fields.  The fused loops rotate the roles of (vₖ₋₁, vₖ), (uₖ₋₁, uₖ) and (wₖ₋₃, wₖ₋₂), and `vector(name)`
    follows the role (khip_trilqr_vector): after k iterations a name holds what the reference's variable of that name holds.  A
    rectangular system (m ≠ n) runs the primitive sequence whatever `fused` says: `last_path` reports 0."""
    _prefix = "trilqr"
    VECTORS = ("u_prev", "u", "p", "dbar", "x", "v_prev", "v", "q", "y", "w_prev3", "w_prev2")
    ROW_SIDE = ("v_prev", "v", "q", "y", "w_prev3", "w_prev2", "dy")            # m entries; every other vector has n
    SOLUTIONS = ("x", "y")

    @property
    def stats(self) -> AdjointStats:
        sp, sd, np_, nd = _int(), _int(), _int(), _int()
        rp, rd, status = c_double_p(), c_double_p(), C.c_char_p()
        _ck(lib().khip_trilqr_adjoint_stats(self._h, C.byref(sp), C.byref(sd), C.byref(rp), C.byref(np_), C.byref(rd), C.byref(nd),
                                            C.byref(status)))
        st = AdjointStats(lib().khip_trilqr_stats(self._h).contents, sp.value, sd.value,
                          np.array(rp[:np_.value]) if np_.value else np.zeros(0), np.array(rd[:nd.value]) if nd.value else np.zeros(0),
                          (status.value or b"").decode("utf-8"))
        if self.adopted:
            st.allocation_timer += self._alloc_s
        st.timer += getattr(self, "_timer_extra", 0.0)
        return st


class TricgWorkspace(_TwoSidedWorkspace):
    """TricgWorkspace(m, n, Sm, Sn) (src/krylov_workspaces.jl), M = N = I: y, uₖ₋₁, uₖ, p, gy₂ₖ₋₁, gy₂ₖ of n entries and x, vₖ₋₁, vₖ, q,
    gx₂ₖ₋₁, gx₂ₖ of m; Δx ("dx", m) and Δy ("dy", n) stay empty until a warm start.  x is on the ROW side (m entries), unlike in
    usymqr!, usymlq! and trilqr!.  The fused loops rotate the roles of (vₖ₋₁, vₖ), (uₖ₋₁, uₖ), (gx₂ₖ₋₁, gx₂ₖ) and (gy₂ₖ₋₁, gy₂ₖ), and
    `vector(name)` follows the role (khip_tricg_vector): after k iterations a name holds what the reference's variable of that name
    holds, except "q" and "p", which the fused loops leave undivided.  A rectangular system (m ≠ n) runs the primitive sequence
    whatever `fused` says: `last_path` reports 0."""
    _prefix = "tricg"
    VECTORS = ("y", "u_prev", "u", "p", "gy_prev", "gy", "x", "v_prev", "v", "q", "gx_prev", "gx")
    ROW_SIDE = ("x", "v_prev", "v", "q", "gx_prev", "gx", "dx")                 # m entries; every other vector has n
    SOLUTIONS = ("x", "y")


class TrimrWorkspace(_TwoSidedWorkspace):
    """TrimrWorkspace(m, n, Sm, Sn) (src/krylov_workspaces.jl), M = N = I: y, uₖ₋₁, uₖ, p, gy₂ₖ₋₃, gy₂ₖ₋₂, gy₂ₖ₋₁, gy₂ₖ of n entries and x, vₖ₋₁,
    vₖ, q, gx₂ₖ₋₃, gx₂ₖ₋₂, gx₂ₖ₋₁, gx₂ₖ of m; Δx ("dx", m) and Δy ("dy", n) stay empty until a warm start.  x is on the ROW side (m
    entries), as in tricg!.  The fused loops rotate the roles of (vₖ₋₁, vₖ), (uₖ₋₁, uₖ) and of the older and the newer pair of g of each
    side, (g₂ₖ₋₃, g₂ₖ₋₂) and (g₂ₖ₋₁, g₂ₖ), and `vector(name)` follows the role (khip_trimr_vector): after k iterations a name holds what
    the reference's variable of that name holds, except "q" and "p", which the fused loops leave undivided.  A rectangular system
    (m ≠ n) runs the primitive sequence whatever `fused` says: `last_path` reports 0."""
    _prefix = "trimr"
    VECTORS = ("y", "u_prev", "u", "p", "gy_m3", "gy_m2", "gy_m1", "gy", "x", "v_prev", "v", "q", "gx_m3", "gx_m2", "gx_m1", "gx")
    ROW_SIDE = ("x", "v_prev", "v", "q", "gx_m3", "gx_m2", "gx_m1", "gx", "dx")                 # m entries; every other vector has n
    SOLUTIONS = ("x", "y")


class UsymlqrWorkspace(_TwoSidedWorkspace):
    """UsymlqrWorkspace(m, n, Sm, Sn) (src/krylov_workspaces.jl): r, x of m entries, y, z of n, vₖ₋₁, vₖ of m, uₖ₋₁, uₖ, p of n, q, d̅ of m
    and wₖ₋₂, wₖ₋₁ of n; Δx ("dx", m) and Δy ("dy", n) stay empty until a warm start.  x is on the ROW side (m entries), as in tricg!.
    stats carries Aresiduals.  The fused loops rotate the roles of (vₖ₋₁, vₖ), (uₖ₋₁, uₖ) and (wₖ₋₂, wₖ₋₁), and `vector(name)` follows the role
    (khip_usymlqr_vector): after k iterations a name holds what the reference's variable of that name holds.  A rectangular system
    (m ≠ n) runs the primitive sequence whatever `fused` says: `last_path` reports 0."""
    _prefix = "usymlqr"
    VECTORS = ("r", "x", "y", "z", "v_prev", "v", "u_prev", "u", "p", "q", "dbar", "w_m2", "w_m1")
    ROW_SIDE = ("r", "x", "v_prev", "v", "q", "dbar", "dx")                             # m entries; every other vector has n
    SOLUTIONS = ("x", "y")
    ARESIDUALS = True


class CgsWorkspace(_BiLanczosWorkspace):
    """CgsWorkspace(m, n, S) (src/krylov_workspaces.jl): x, r, u, p, q, ts; Δx, yz, vw stay empty until needed.  cgs! rotates no
    roles: every name keeps its buffer."""
    _prefix = "cgs"
    VECTORS = ("x", "r", "u", "p", "q", "ts")


class SymmlqWorkspace(_Workspace):
    """SymmlqWorkspace(m, n, S; window = 5) (src/krylov_workspaces.jl:461-476): x, Mvold, Mv, Mv_next, w̅ ("wbar"); Δx and v stay
    empty until needed.  stats carries residualscg, errors, errorscg (NaN where the reference has `missing`), Anorm and Acond.  The
    fused loops rotate the roles of (Mvold, Mv, Mv_next), and `vector(name)` follows the role (khip_symmlq_vector): after a solve
    a name holds what the reference's variable of that name holds."""
    _prefix = "symmlq"
    VECTORS = ("x", "Mvold", "Mv", "Mv_next", "wbar")

    def __init__(self, ctx: Context, m: int, n: int, window: int = 5, adopt: bool | None = None, vectors=None):
        self.ctx, self.m, self.n, self.window = ctx, m, n, window
        self.adopted = vectors is not None or (_adopt_default() if adopt is None else bool(adopt))
        self._h = C.c_void_p()
        if self.adopted:
            t0 = time.perf_counter()
            self._vec = dict(vectors) if vectors is not None else {k: ctx.empty(n) for k in self.VECTORS}     # dx, v stay empty
            self._alloc_s = time.perf_counter() - t0
            _ck(lib().khip_symmlq_workspace_adopt(ctx._h, m, n, window, *[self._vec[k].ptr for k in self.VECTORS], C.byref(self._h)))
        else:
            _ck(lib().khip_symmlq_workspace_create(ctx._h, m, n, window, C.byref(self._h)))

    @property
    def stats(self) -> SimpleStats:
        st = super().stats
        ptr = [c_double_p() for _ in range(3)]
        cnt = [_int() for _ in range(3)]
        _ck(lib().khip_symmlq_histories(self._h, C.byref(ptr[0]), C.byref(cnt[0]), C.byref(ptr[1]), C.byref(cnt[1]),
                                        C.byref(ptr[2]), C.byref(cnt[2])))
        for name, q, k in zip(("residualscg", "errors", "errorscg"), ptr, cnt):
            setattr(st, name, np.array(q[:k.value]) if k.value else np.zeros(0))
        an, ac = C.c_double(), C.c_double()
        _ck(lib().khip_symmlq_norms(self._h, C.byref(an), C.byref(ac)))
        st.Anorm, st.Acond = an.value, ac.value
        return st

    def vector(self, name: str):
        if name == "x":
            return self.x
        p = lib().khip_symmlq_vector(self._h, name.encode())
        return DeviceVector(self.ctx, self.n, ptr=p, owner=self) if p else None


class MinresQlpWorkspace(_Workspace):
    """MinresQlpWorkspace(m, n, S) (src/krylov_workspaces.jl:713-768): x, wₖ₋₁, wₖ, M⁻¹vₖ₋₁, M⁻¹vₖ, p ("wkm1", "wk", "Mvkm1", "Mvk");
    Δx and vₖ ("dx", "vk") stay empty until needed.  stats carries Aresiduals and Acond (one entry more than Aresiduals).  The fused
    loops rotate the roles of (Mvkm1, Mvk, p) and swap those of (wkm1, wk), and `vector(name)` follows the role
    (khip_minres_qlp_vector): after a solve a name holds what the reference's variable of that name holds."""
    _prefix = "minres_qlp"
    VECTORS = ("x", "wkm1", "wk", "Mvkm1", "Mvk", "p")

    def __init__(self, ctx: Context, m: int, n: int, adopt: bool | None = None, vectors=None):
        self.ctx, self.m, self.n = ctx, m, n
        self.adopted = vectors is not None or (_adopt_default() if adopt is None else bool(adopt))
        self._h = C.c_void_p()
        if self.adopted:
            t0 = time.perf_counter()
            self._vec = dict(vectors) if vectors is not None else {k: ctx.empty(n) for k in self.VECTORS}     # dx, vk stay empty
            self._alloc_s = time.perf_counter() - t0
            _ck(lib().khip_minres_qlp_workspace_adopt(ctx._h, m, n, *[self._vec[k].ptr for k in self.VECTORS], C.byref(self._h)))
        else:
            _ck(lib().khip_minres_qlp_workspace_create(ctx._h, m, n, C.byref(self._h)))

    @property
    def stats(self) -> SimpleStats:
        st = super().stats
        ar, nar, ac, nac = c_double_p(), _int(), c_double_p(), _int()
        _ck(lib().khip_minres_qlp_histories(self._h, C.byref(ar), C.byref(nar), C.byref(ac), C.byref(nac)))
        st.Aresiduals = np.array(ar[:nar.value]) if nar.value else np.zeros(0)
        st.Acond = np.array(ac[:nac.value]) if nac.value else np.zeros(0)
        return st

    @property
    def fused_product(self) -> bool:
        """The last solve's Lanczos step ran inside the sliced SpMV (khip_minres_qlp_fused_product)."""
        return lib().khip_minres_qlp_fused_product(self._h) == 1

    def vector(self, name: str):
        if name == "x":
            return self.x
        p = lib().khip_minres_qlp_vector(self._h, name.encode())
        return DeviceVector(self.ctx, self.n, ptr=p, owner=self) if p else None


class BilqrWorkspace(_BiLanczosWorkspace):
    """BilqrWorkspace(m, n, S) (src/krylov_workspaces.jl:1818-1836): uₖ₋₁, uₖ, q, vₖ₋₁, vₖ, p, x, y, d̅, wₖ₋₃, wₖ₋₂; Δx and Δy stay empty
    until a warm start."""
    _prefix = "bilqr"
    VECTORS = ("u_prev", "u", "q", "v_prev", "v", "p", "x", "y", "dbar", "w_prev3", "w_prev2")
    SOLUTIONS = ("x", "y")

    @property
    def x(self) -> DeviceVector:
        if self.adopted:
            return self._vec["x"]
        return DeviceVector(self.ctx, self.n, ptr=lib().khip_bilqr_solution_x(self._h), owner=self)

    @property
    def y(self) -> DeviceVector:
        if self.adopted:
            return self._vec["y"]
        return DeviceVector(self.ctx, self.n, ptr=lib().khip_bilqr_solution_y(self._h), owner=self)

    @property
    def stats(self) -> AdjointStats:
        sp, sd, np_, nd = _int(), _int(), _int(), _int()
        rp, rd, status = c_double_p(), c_double_p(), C.c_char_p()
        _ck(lib().khip_bilqr_adjoint_stats(self._h, C.byref(sp), C.byref(sd), C.byref(rp), C.byref(np_), C.byref(rd), C.byref(nd),
                                           C.byref(status)))
        st = AdjointStats(lib().khip_bilqr_stats(self._h).contents, sp.value, sd.value,
                          np.array([rp[i] for i in range(np_.value)]), np.array([rd[i] for i in range(nd.value)]),
                          (status.value or b"").decode("utf-8"))
        if self.adopted:
            st.allocation_timer += self._alloc_s
        st.timer += getattr(self, "_timer_extra", 0.0)
        return st

    def warm_start_(self, x0: DeviceVector, y0: DeviceVector | None = None):
        """warm_start!(workspace, x0, y0) (src/workspace_accessors.jl): Δx and Δy are allocated on first need; both are required."""
        if y0 is None or x0 is None:
            raise KhipError(-1, "bilqr: warm_start needs x0 and y0")
        if self.adopted:
            self._allocate_if(True, "dx")
            self._allocate_if(True, "dy")
            kcopy_(self.n, self._vec["dx"], x0)
            kcopy_(self.n, self._vec["dy"], y0)
            _ck(lib().khip_bilqr_warm_start(self._h, self._vec["dx"].ptr, self._vec["dy"].ptr))     # same pointers: only the flag
        else:
            _ck(lib().khip_bilqr_warm_start(self._h, _p(x0), _p(y0)))
        return self


def _finish(ws, rc):
    ws._timer_extra = 0.0          # an entry point that did work of its own before the solve adds it afterwards
    if rc != 0:
        st = ws.stats
        raise KhipError(rc, st.error or lib().khip_last_error().decode("utf-8", "replace"))
    return ws


def cg_(ws: CgWorkspace, A, b: DeviceVector, M=None, **kw):
    """cg!(workspace, A, b; M, radius, linesearch, atol, rtol, itmax, timemax, history, callback)
    (src/cg.jl:120-291).  Returns the workspace."""
    keep = []
    ws._allocate_if(M is not None, "z")                                                   # src/cg.jl:142
    ws._allocate_if(bool(kw.get("linesearch")) or kw.get("radius", 0.0) > 0, "npc_dir")    # :143
    opts = _make_options(keep=keep, ws=ws, **kw)
    rc = lib().khip_cg_solve(ws._h, _make_operator(ws.ctx, A, ws.n, keep), _make_operator(ws.ctx, M, ws.n, keep),
                             _p(b), C.byref(opts))
    return _finish(ws, rc)


def gmres_(ws: GmresWorkspace, A, b: DeviceVector, M=None, N=None, **kw):
    """gmres!(workspace, A, b; M, N, restart, reorthogonalization, ...) (src/gmres.jl:121-384)."""
    keep = []
    ws._allocate_if(M is not None, "q")                                                   # src/gmres.jl:142-144
    ws._allocate_if(N is not None, "p")
    ws._allocate_if(bool(kw.get("restart")), "dx")
    opts = _make_options(keep=keep, ws=ws, **kw)
    rc = lib().khip_gmres_solve(ws._h, _make_operator(ws.ctx, A, ws.n, keep), _make_operator(ws.ctx, M, ws.n, keep),
                                _make_operator(ws.ctx, N, ws.n, keep), _p(b), C.byref(opts))
    return _finish(ws, rc)


def bicgstab_(ws: BicgstabWorkspace, A, b: DeviceVector, c: DeviceVector | None = None, M=None, N=None, **kw):
    """bicgstab!(workspace, A, b; c, M, N, ...) (src/bicgstab.jl:125-277)."""
    keep = []
    ws._allocate_if(M is not None, "t")                                                   # src/bicgstab.jl:148-149
    ws._allocate_if(N is not None, "yz")
    opts = _make_options(keep=keep, ws=ws, **kw)
    rc = lib().khip_bicgstab_solve(ws._h, _make_operator(ws.ctx, A, ws.n, keep),
                                   _make_operator(ws.ctx, M, ws.n, keep), _make_operator(ws.ctx, N, ws.n, keep),
                                   _p(b), _p(c), C.byref(opts))
    return _finish(ws, rc)


def cgs_(ws: CgsWorkspace, A, b: DeviceVector, c: DeviceVector | None = None, M=None, N=None, **kw):
    """cgs!(workspace, A, b; c, M, N, ldiv, atol, rtol, itmax, timemax, verbose, history, callback, iostream)
    (src/cgs.jl:126-281).  Returns the workspace."""
    keep = []
    if len(b) != ws.n:
        raise KhipError(-1, "Inconsistent problem size")                                  # src/cgs.jl:135
    ws._allocate_if(M is not None, "vw")                                                # src/cgs.jl:148-149
    ws._allocate_if(N is not None, "yz")
    opts = _make_options(keep=keep, ws=ws, **kw)
    rc = lib().khip_cgs_solve(ws._h, _make_operator(ws.ctx, A, ws.n, keep), _make_operator(ws.ctx, M, ws.n, keep),
                              _make_operator(ws.ctx, N, ws.n, keep), _p(b), _p(c), C.byref(opts))
    return _finish(ws, rc)


def minres_(ws: MinresWorkspace, A, b: DeviceVector, M=None, λ=0.0, etol=None, conlim=None, **kw):
    """minres!(workspace, A, b; M, ldiv, linesearch, λ, atol, rtol, etol, conlim, itmax, timemax, verbose, history, callback,
    iostream) (src/minres.jl:164-484).  linesearch = true is refused (KHIP_ERR_UNSUPPORTED).  Returns the workspace."""
    keep = []
    ws._allocate_if(M is not None, "v")                                                   # src/minres.jl:192
    opts = _make_options(keep=keep, ws=ws, **kw)
    prm = lib().khip_minres_default_params()
    prm.lambda_ = float(λ)
    if etol is not None:
        prm.etol = etol
    if conlim is not None:
        prm.conlim = conlim
    rc = lib().khip_minres_solve(ws._h, _make_operator(ws.ctx, A, ws.n, keep), _make_operator(ws.ctx, M, ws.n, keep), _p(b),
                                 C.byref(opts), C.byref(prm))
    return _finish(ws, rc)


def symmlq_(ws: SymmlqWorkspace, A, b: DeviceVector, M=None, transfer_to_cg=True, λ=0.0, λest=0.0, etol=None, conlim=None, **kw):
    """symmlq!(workspace, A, b; M, ldiv, transfer_to_cg, λ, λest, atol, rtol, etol, conlim, itmax, timemax, verbose, history,
    callback, iostream) (src/symmlq.jl:132-464).  Returns the workspace."""
    keep = []
    if len(b) != ws.n:
        raise KhipError(-1, "Inconsistent problem size")                                  # src/symmlq.jl:141
    ws._allocate_if(M is not None, "v")                                                   # src/symmlq.jl:152
    opts = _make_options(keep=keep, ws=ws, **kw)
    prm = lib().khip_symmlq_default_params()
    prm.lambda_ = float(λ)
    prm.lambda_est = float(λest)
    prm.transfer_to_cg = int(bool(transfer_to_cg))
    if etol is not None:
        prm.etol = etol
    if conlim is not None:
        prm.conlim = conlim
    rc = lib().khip_symmlq_solve(ws._h, _make_operator(ws.ctx, A, ws.n, keep), _make_operator(ws.ctx, M, ws.n, keep), _p(b),
                                 C.byref(opts), C.byref(prm))
    return _finish(ws, rc)


def minres_qlp_(ws: MinresQlpWorkspace, A, b: DeviceVector, M=None, λ=0.0, Artol=None, **kw):
    """minres_qlp!(workspace, A, b; M, ldiv, linesearch, λ, atol, rtol, Artol, itmax, timemax, verbose, history, callback, iostream)
    (src/minres_qlp.jl:131-538).  linesearch = true is refused (KHIP_ERR_UNSUPPORTED).  Returns the workspace."""
    keep = []
    if len(b) != ws.n:
        raise KhipError(-1, "Inconsistent problem size")                                  # src/minres_qlp.jl:140
    ws._allocate_if(M is not None, "vk")                                                  # src/minres_qlp.jl:152
    opts = _make_options(keep=keep, ws=ws, **kw)
    prm = lib().khip_minres_qlp_default_params()
    prm.lambda_ = float(λ)
    if Artol is not None:
        prm.Artol = Artol
    rc = lib().khip_minres_qlp_solve(ws._h, _make_operator(ws.ctx, A, ws.n, keep), _make_operator(ws.ctx, M, ws.n, keep), _p(b),
                                     C.byref(opts), C.byref(prm))
    return _finish(ws, rc)


def cg_lanczos_shift_(ws: CgLanczosShiftWorkspace, A, b: DeviceVector, shifts, M=None, ldiv=False, check_curvature=False, **kw):
    """cg_lanczos_shift!(workspace, A, b, shifts; M, ldiv, check_curvature, atol, rtol, itmax, timemax, verbose, history, callback,
    iostream) (src/cg_lanczos_shift.jl:107-284).  Returns the workspace."""
    keep = []
    if len(b) != ws.n:
        raise KhipError(-1, "Inconsistent problem size")
    sh = np.ascontiguousarray(shifts, dtype=np.float64).ravel()
    if len(sh) != ws.nshifts:
        raise KhipError(-1, f"workspace.nshifts = {ws.nshifts} is inconsistent with length(shifts) = {len(sh)}")
    ws._allocate_if(M is not None, "v")                                                   # src/cg_lanczos_shift.jl:133
    opts = _make_options(keep=keep, ws=ws, ldiv=ldiv, **kw)
    prm = lib().khip_cg_lanczos_shift_default_params()
    prm.shifts = sh.ctypes.data_as(c_double_p)
    prm.nshifts = len(sh)
    prm.check_curvature = int(bool(check_curvature))
    rc = lib().khip_cg_lanczos_shift_solve(ws._h, _make_operator(ws.ctx, A, ws.n, keep), _make_operator(ws.ctx, M, ws.n, keep),
                                           _p(b), C.byref(opts), C.byref(prm))
    return _finish(ws, rc)


def _adjoint_of(A, solver: str = "bilq"):
    """A' of a CsrMatrix, built once (khip_csr_transpose) and kept on the object; any other operator must bring its own."""
    if not isinstance(A, CsrMatrix):
        raise KhipError(-1, f"{solver}: a matrix-free A needs its adjoint passed as At")
    At = getattr(A, "_adjoint", None)
    if At is None:
        At = A.transpose()
        A._adjoint = At
    return At


def _bilq_precond_adjoint(name: str, op, adjoint, solver: str = "bilq"):
    """The adjoint bilq! or qmr! (`solver`) applies for the preconditioner `op` (M or N): the one given, else `op` itself where that is right -- the
    identity (None) and Jacobi (diagonal).  ILU(0) of a nonsymmetric A or a callable is not its own adjoint: without an explicit
    adjoint the solve would run N A' M in place of N' A' M' and still report convergence, so it is refused."""
    if op is None or adjoint is not None or isinstance(op, Jacobi):
        return adjoint
    raise KhipError(-1, f"{solver}: {name} = {type(op).__name__} is not known to be its own adjoint: pass {name}t (the operator "
                        f"y <- {name}' x), or use a Jacobi {name}")


def _bilq_qmr_solve(ws, prm, A, b, c, M, N, At, Mt, Nt, kw):
    """What bilq_ and qmr_ share: the adjoints (At defaults to A.transpose(), Mt / Nt to a Jacobi M / N itself), the size check, t
    and s on first need (src/bilq.jl:145-146, src/qmr.jl:151-152), Mt / Nt into the solver's params `prm`, and the call."""
    keep = []
    solver = ws._prefix
    Mt = _bilq_precond_adjoint("M", M, Mt, solver=solver)
    Nt = _bilq_precond_adjoint("N", N, Nt, solver=solver)
    if len(b) != ws.n:
        raise KhipError(-1, "Inconsistent problem size")
    if At is None:
        At = _adjoint_of(A, solver=solver)
    ws._allocate_if(M is not None, "t")
    ws._allocate_if(N is not None, "s")
    opts = _make_options(keep=keep, ws=ws, **kw)
    if Mt is not None:
        prm.Mt = C.cast(_make_operator(ws.ctx, Mt, ws.n, keep), C.POINTER(COperator))
    if Nt is not None:
        prm.Nt = C.cast(_make_operator(ws.ctx, Nt, ws.n, keep), C.POINTER(COperator))
    rc = ws._fn("solve")(ws._h, _make_operator(ws.ctx, A, ws.n, keep), _make_operator(ws.ctx, At, ws.n, keep),
                         _make_operator(ws.ctx, M, ws.n, keep), _make_operator(ws.ctx, N, ws.n, keep), _p(b), _p(c),
                         C.byref(opts), C.byref(prm))
    return _finish(ws, rc)


def bilq_(ws: BilqWorkspace, A, b: DeviceVector, c: DeviceVector | None = None, transfer_to_bicg=True, M=None, N=None, At=None,
          Mt=None, Nt=None, **kw):
    """bilq!(workspace, A, b; c, transfer_to_bicg, M, N, ldiv, atol, rtol, itmax, timemax, verbose, history, callback, iostream)
    (src/bilq.jl:118-407).  At: the adjoint of A (default: A.transpose(), cached on A); Mt / Nt: the adjoints of M / N, required
    unless the operator is a Jacobi (its own adjoint).  Returns the workspace."""
    prm = lib().khip_bilq_default_params()
    prm.transfer_to_bicg = int(bool(transfer_to_bicg))
    return _bilq_qmr_solve(ws, prm, A, b, c, M, N, At, Mt, Nt, kw)


def qmr_(ws: QmrWorkspace, A, b: DeviceVector, c: DeviceVector | None = None, M=None, N=None, At=None, Mt=None, Nt=None, **kw):
    """qmr!(workspace, A, b; c, M, N, ldiv, atol, rtol, itmax, timemax, verbose, history, callback, iostream)
    (src/qmr.jl:124-406).  At: the adjoint of A (default: A.transpose(), cached on A); Mt / Nt: the adjoints of M / N, required
    unless the operator is a Jacobi (its own adjoint).  Returns the workspace."""
    return _bilq_qmr_solve(ws, lib().khip_qmr_default_params(), A, b, c, M, N, At, Mt, Nt, kw)


def _ssy_solve(ws, A, b, c, At, opts_kw, prm=None, c_message="the starting vector of the second Krylov space"):
    """What the six solvers on the Saunders-Simon-Yip process share: c is required (`c_message` says what it is), b has m entries
    and c has n, At defaults to A.transpose(), a matrix-free operator is wrapped at its two lengths, and the call; `prm` is the
    solver's params (usymqr! has none)."""
    keep = []
    solver = ws._prefix
    if c is None:
        raise KhipError(-1, f"{solver}: c ({c_message}) is required")
    if len(b) != ws.m or len(c) != ws.n:
        raise KhipError(-1, "Inconsistent problem size")
    if At is None:
        At = _adjoint_of(A, solver=solver)
    opts = _make_options(keep=keep, ws=ws, **opts_kw)

    def operator(op, nin, nout):
        if op is None or isinstance(op, CsrMatrix):
            return _make_operator(ws.ctx, op, nin, keep)
        return _make_operator_mn(ws.ctx, op, nin, nout, keep)
    params = () if prm is None else (C.byref(prm),)
    rc = ws._fn("solve")(ws._h, operator(A, ws.n, ws.m), operator(At, ws.m, ws.n), _p(b), _p(c), C.byref(opts), *params)
    return _finish(ws, rc)


def usymqr_(ws: UsymqrWorkspace, A, b: DeviceVector, c: DeviceVector | None = None, At=None, **kw):
    """usymqr!(workspace, A, b, c; atol, rtol, itmax, timemax, verbose, history, callback, iostream) (src/usymqr.jl:130-365) for A of m
    rows and n columns, b of m entries and c of n.  At: the adjoint of A (default: A.transpose(), built once and kept on A); a
    matrix-free A is callable(x[n], y[m]) and brings At = callable(x[m], y[n]).  Returns the workspace."""
    return _ssy_solve(ws, A, b, c, At, kw)


def usymlq_(ws: UsymlqWorkspace, A, b: DeviceVector, c: DeviceVector | None = None, At=None, transfer_to_usymcg=True, **kw):
    """usymlq!(workspace, A, b, c; transfer_to_usymcg, atol, rtol, itmax, timemax, verbose, history, callback, iostream)
    (src/usymlq.jl:124-366) for A of m rows and n columns, b of m entries and c of n.  At: the adjoint of A (default: A.transpose(),
    built once and kept on A); a matrix-free A is callable(x[n], y[m]) and brings At = callable(x[m], y[n]).  Returns the workspace."""
    prm = lib().khip_usymlq_default_params()
    prm.transfer_to_usymcg = int(bool(transfer_to_usymcg))
    return _ssy_solve(ws, A, b, c, At, kw, prm)


def trilqr_(ws: TrilqrWorkspace, A, b: DeviceVector, c: DeviceVector | None = None, At=None, transfer_to_usymcg=True, **kw):
    """trilqr!(workspace, A, b, c; transfer_to_usymcg, atol, rtol, itmax, timemax, verbose, history, callback, iostream)
    (src/trilqr.jl:115-460): x of A x = b by USYMLQ and t of Aᴴ t = c by USYMQR from one orthogonal tridiagonalisation, for A of m rows
    and n columns, b of m entries and c of n.  At: the adjoint of A (default: A.transpose(), built once and kept on A); a matrix-free
    A is callable(x[n], y[m]) and brings At = callable(x[m], y[n]).  Returns the workspace."""
    prm = lib().khip_trilqr_default_params()
    prm.transfer_to_usymcg = int(bool(transfer_to_usymcg))
    return _ssy_solve(ws, A, b, c, At, kw, prm, c_message="the right-hand side of the dual system")


def tricg_(ws: TricgWorkspace, A, b: DeviceVector, c: DeviceVector | None = None, At=None, τ=1.0, ν=-1.0, spd=False, snd=False,
           flip=False, M=None, N=None, ldiv=False, **kw):
    """tricg!(workspace, A, b, c; spd, snd, flip, τ, ν, atol, rtol, itmax, timemax, verbose, history, callback, iostream)
    (src/tricg.jl:149-484): [τI A; Aᴴ νI] [x; y] = [b; c] for A of m rows and n columns, b of m entries and c of n; M = N = I only.
    At: the adjoint of A (default: A.transpose(), built once and kept on A); a matrix-free A is callable(x[n], y[m]) and brings
    At = callable(x[m], y[n]).  Returns the workspace."""
    if c is not None and (M is not None or N is not None):                      # a missing c is reported first, by _ssy_solve
        raise KhipError(-5, "tricg: M and N other than I are not supported")
    prm = lib().khip_tricg_default_params()
    prm.tau, prm.nu = float(τ), float(ν)
    prm.spd, prm.snd, prm.flip = int(bool(spd)), int(bool(snd)), int(bool(flip))
    return _ssy_solve(ws, A, b, c, At, kw, prm, c_message="the second right-hand side")


def trimr_(ws: TrimrWorkspace, A, b: DeviceVector, c: DeviceVector | None = None, At=None, τ=1.0, ν=-1.0, spd=False, snd=False,
           flip=False, sp=False, M=None, N=None, ldiv=False, **kw):
    """trimr!(workspace, A, b, c; spd, snd, flip, sp, τ, ν, atol, rtol, itmax, timemax, verbose, history, callback, iostream)
    (src/trimr.jl:150-577): [τI A; Aᴴ νI] [x; y] = [b; c] for A of m rows and n columns, b of m entries and c of n; M = N = I only.
    At: the adjoint of A (default: A.transpose(), built once and kept on A); a matrix-free A is callable(x[n], y[m]) and brings
    At = callable(x[m], y[n]).  Returns the workspace."""
    if c is not None and (M is not None or N is not None):                      # a missing c is reported first, by _ssy_solve
        raise KhipError(-5, "trimr: M and N other than I are not supported")
    prm = lib().khip_trimr_default_params()
    prm.tau, prm.nu = float(τ), float(ν)
    prm.spd, prm.snd, prm.flip, prm.sp = int(bool(spd)), int(bool(snd)), int(bool(flip)), int(bool(sp))
    return _ssy_solve(ws, A, b, c, At, kw, prm, c_message="the second right-hand side")


def usymlqr_(ws: UsymlqrWorkspace, A, b: DeviceVector, c: DeviceVector | None = None, At=None, ls=True, ln=True, ldiv=False, **kw):
    """usymlqr!(workspace, A, b, c; ls, ln, ldiv, atol, rtol, itmax, timemax, verbose, history, callback, iostream)
    (src/usymlqr.jl:136-509): [I A; Aᴴ 0] [x; y] = [b; c] for A of m rows and n columns, b of m entries and c of n, as the sum of a
    least-squares problem (ls) and a least-norm problem (ln).  `ldiv` is accepted and ignored (there are no preconditioners).
    At: the adjoint of A (default: A.transpose(), built once and kept on A); a matrix-free A is callable(x[n], y[m]) and brings
    At = callable(x[m], y[n]).  Returns the workspace."""
    prm = lib().khip_usymlqr_default_params()
    prm.ls, prm.ln = int(bool(ls)), int(bool(ln))
    return _ssy_solve(ws, A, b, c, At, kw, prm, c_message="the second right-hand side")


def bilqr_(ws: BilqrWorkspace, A, b: DeviceVector, c: DeviceVector | None = None, At=None, transfer_to_bicg=True, **kw):
    """bilqr!(workspace, A, b, c; transfer_to_bicg, atol, rtol, itmax, timemax, verbose, history, callback, iostream)
    (src/bilqr.jl:116-484): x of A x = b by BiLQ and y of A' y = c by QMR from one two-sided Lanczos process.  At: the adjoint of A
    (default: A.transpose(), cached on A).  Returns the workspace."""
    keep = []
    if c is None:
        raise KhipError(-1, "bilqr: c (the right-hand side of the dual system) is required")
    if len(b) != ws.n or len(c) != ws.n:
        raise KhipError(-1, "Inconsistent problem size")
    if At is None:
        At = _adjoint_of(A, solver="bilqr")
    opts = _make_options(keep=keep, ws=ws, **kw)
    prm = lib().khip_bilqr_default_params()
    prm.transfer_to_bicg = int(bool(transfer_to_bicg))
    rc = lib().khip_bilqr_solve(ws._h, _make_operator(ws.ctx, A, ws.n, keep), _make_operator(ws.ctx, At, ws.n, keep), _p(b), _p(c),
                                C.byref(opts), C.byref(prm))
    return _finish(ws, rc)


def _local_rows(A):
    return A.m if isinstance(A, CsrMatrix) else None


# ---- the generated entry points of src/interface.jl, with what they FORWARD -----------------------------------------------------
# def_kwargs_cg / _gmres / _bicgstab / _block_gmres (src/cg.jl:101-112, src/gmres.jl:96-110, src/bicgstab.jl:105-116,
# src/block_gmres.jl:85-99) as this mirror spells them (M / N: None = I; iostream: None = kstdout; timemax: inf).  Every
# out-of-place and generic entry below builds the complete keyword set from these tables and passes ALL of it on, as the reference's
# generated methods do -- tests/test_abi.py compares the tables with the reference's, and test_gpu_adopt.py asserts that the solve
# they lead to ran the device-resident loop (`last_path == 2`).
_SQRT_EPS = math.sqrt(np.finfo(np.float64).eps)
FORWARDED_DEFAULTS = {
    "cg": dict(M=None, ldiv=False, radius=0.0, linesearch=False, atol=_SQRT_EPS, rtol=_SQRT_EPS, itmax=0, timemax=math.inf,
               verbose=0, history=False, callback=default_callback, iostream=None),
    "gmres": dict(M=None, N=None, ldiv=False, restart=False, reorthogonalization=False, atol=_SQRT_EPS, rtol=_SQRT_EPS, itmax=0,
                  timemax=math.inf, verbose=0, history=False, callback=default_callback, iostream=None),
    "bicgstab": dict(c=None, M=None, N=None, ldiv=False, atol=_SQRT_EPS, rtol=_SQRT_EPS, itmax=0, timemax=math.inf, verbose=0,
                     history=False, callback=default_callback, iostream=None),
    "block_gmres": dict(M=None, N=None, ldiv=False, restart=False, reorthogonalization=False, atol=_SQRT_EPS, rtol=_SQRT_EPS, itmax=0,
                        timemax=math.inf, verbose=0, history=False, callback=default_callback, iostream=None),
    "minres": dict(M=None, ldiv=False, linesearch=False, λ=0.0, atol=_SQRT_EPS, rtol=_SQRT_EPS, etol=_SQRT_EPS,
                   conlim=1.0 / _SQRT_EPS, itmax=0, timemax=math.inf, verbose=0, history=False, callback=default_callback,
                   iostream=None),
    "cg_lanczos_shift": dict(M=None, ldiv=False, check_curvature=False, atol=_SQRT_EPS, rtol=_SQRT_EPS, itmax=0, timemax=math.inf,
                             verbose=0, history=False, callback=default_callback, iostream=None),
    "bilq": dict(c=None, transfer_to_bicg=True, M=None, N=None, ldiv=False, atol=_SQRT_EPS, rtol=_SQRT_EPS, itmax=0,
                 timemax=math.inf, verbose=0, history=False, callback=default_callback, iostream=None),
    "qmr": dict(c=None, M=None, N=None, ldiv=False, atol=_SQRT_EPS, rtol=_SQRT_EPS, itmax=0, timemax=math.inf, verbose=0,
                history=False, callback=default_callback, iostream=None),
    "cgs": dict(c=None, M=None, N=None, ldiv=False, atol=_SQRT_EPS, rtol=_SQRT_EPS, itmax=0, timemax=math.inf, verbose=0,
                history=False, callback=default_callback, iostream=None),
    "symmlq": dict(M=None, ldiv=False, transfer_to_cg=True, λ=0.0, λest=0.0, atol=_SQRT_EPS, rtol=_SQRT_EPS, etol=_SQRT_EPS,
                   conlim=1.0 / _SQRT_EPS, itmax=0, timemax=math.inf, verbose=0, history=False, callback=default_callback,
                   iostream=None),
    "minres_qlp": dict(M=None, ldiv=False, linesearch=False, λ=0.0, atol=_SQRT_EPS, rtol=_SQRT_EPS, Artol=_SQRT_EPS, itmax=0,
                       timemax=math.inf, verbose=0, history=False, callback=default_callback, iostream=None),
    "bilqr": dict(transfer_to_bicg=True, atol=_SQRT_EPS, rtol=_SQRT_EPS, itmax=0, timemax=math.inf, verbose=0, history=False,
                  callback=default_callback, iostream=None),
    "usymqr": dict(atol=_SQRT_EPS, rtol=_SQRT_EPS, itmax=0, timemax=math.inf, verbose=0, history=False,
                   callback=default_callback, iostream=None),
    "usymlq": dict(transfer_to_usymcg=True, atol=_SQRT_EPS, rtol=_SQRT_EPS, itmax=0, timemax=math.inf, verbose=0, history=False,
                   callback=default_callback, iostream=None),
    "trilqr": dict(transfer_to_usymcg=True, atol=_SQRT_EPS, rtol=_SQRT_EPS, itmax=0, timemax=math.inf, verbose=0, history=False,
                   callback=default_callback, iostream=None),
    "tricg": dict(M=None, N=None, ldiv=False, spd=False, snd=False, flip=False, τ=1.0, ν=-1.0, atol=_SQRT_EPS, rtol=_SQRT_EPS, itmax=0,
                  timemax=math.inf, verbose=0, history=False, callback=default_callback, iostream=None),
    "trimr": dict(M=None, N=None, ldiv=False, spd=False, snd=False, flip=False, sp=False, τ=1.0, ν=-1.0, atol=_SQRT_EPS, rtol=_SQRT_EPS,
                  itmax=0, timemax=math.inf, verbose=0, history=False, callback=default_callback, iostream=None),
    "usymlqr": dict(ls=True, ln=True, ldiv=False, atol=_SQRT_EPS, rtol=_SQRT_EPS, itmax=0, timemax=math.inf, verbose=0, history=False,
                    callback=default_callback, iostream=None),
}
WORKSPACE_KWARGS = {"gmres": dict(memory=20), "block_gmres": dict(memory=5)}      # kwargs_workspace_gmres, _block_gmres
# kwargs_workspace_minres (src/minres.jl:159): kept apart from WORKSPACE_KWARGS, whose contents tests/test_abi.py pins
MINRES_WORKSPACE_KWARGS = dict(window=5)
SYMMLQ_WORKSPACE_KWARGS = dict(window=5)                                        # kwargs_workspace_symmlq (src/symmlq.jl:121)


def _workspace_kwargs(method: str) -> dict:
    if method == "symmlq":
        return SYMMLQ_WORKSPACE_KWARGS
    return MINRES_WORKSPACE_KWARGS if method == "minres" else WORKSPACE_KWARGS.get(method, {})


def _forward(method: str, kw: dict) -> dict:
    """The keyword set a generated entry point passes to the in-place method: its defaults, overridden by what the caller gave.
    Keywords of this library that the reference does not have (fused, variant) pass through."""
    full = dict(FORWARDED_DEFAULTS[method])
    full.update(kw)
    return full


def krylov_workspace(method: str, *args, ctx: Context | None = None, **kw):
    """krylov_workspace(Val(method), m, n, S; memory) / (Val(method), A, b; memory) (src/interface.jl:117-141, 237-244)."""
    cls = {"cg": CgWorkspace, "gmres": GmresWorkspace, "bicgstab": BicgstabWorkspace, "block_gmres": BlockGmresWorkspace,
           "minres": MinresWorkspace, "cg_lanczos_shift": CgLanczosShiftWorkspace, "bilq": BilqWorkspace,
           "qmr": QmrWorkspace, "bilqr": BilqrWorkspace, "cgs": CgsWorkspace,
           "symmlq": SymmlqWorkspace, "minres_qlp": MinresQlpWorkspace, "usymqr": UsymqrWorkspace,
           "usymlq": UsymlqWorkspace, "trilqr": TrilqrWorkspace, "tricg": TricgWorkspace,
           "trimr": TrimrWorkspace, "usymlqr": UsymlqrWorkspace}[method]
    if method in _TAKES_C and len(args) == 3:                                    # (A, b, c): m = length(b), n = length(c)
        A, b, c = args
        return cls(b.ctx, len(b), len(c), **kw)
    if method == "cg_lanczos_shift":                                            # (A, b, nshifts) / (m, n, nshifts)
        if isinstance(args[1], DeviceVector):
            A, b, nshifts = args
            return cls(b.ctx, len(b), len(b), nshifts, **kw)
        m, n, nshifts = args
        return cls(ctx, m, n, nshifts, **kw)
    if len(args) == 2 and isinstance(args[1], DeviceVector):                  # (A, b)
        A, b = args
        return cls(b.ctx, len(b), len(b), **kw)
    if method == "block_gmres":
        if len(args) == 2:                                                       # (A, B) with a host n x p array B
            B = np.asarray(args[1])
            return cls(ctx or args[0].ctx, B.shape[0], B.shape[0], B.shape[1], **kw)
        m, n, p = args
        return cls(ctx, m, n, p, **kw)
    m, n = args
    return cls(ctx, m, n, **kw)


_INPLACE = {}      # filled below: CgWorkspace -> ("cg", cg_), ...
_TAKES_C = {"usymqr", "usymlq", "trilqr", "tricg", "trimr", "usymlqr"}          # krylov_solve(Val(method), A, b, c, ...): A is m x n
_TAKES_X0_Y0 = {"tricg", "trimr", "usymlqr"}       # ... and krylov_solve takes (x0, y0) and returns (x, y, stats, workspace)


def krylov_solve_(ws, A, b, x0=None, **kw):
    """krylov_solve!(workspace, A, b[, x0]; kwargs...) (src/interface.jl:331-345, 306-320): dispatch on the workspace type; the x0
    form warm-starts first and charges that time to the solve, as the reference does."""
    method, inplace = _INPLACE[type(ws)]
    if method == "cg_lanczos_shift":                                            # krylov_solve!(ws, A, b, shifts; kwargs...)
        shifts = x0 if x0 is not None else kw.pop("shifts")
        inplace(ws, A, b, shifts, **_forward(method, kw))
        ws._timer_extra = 0.0
        return ws
    full = _forward(method, kw)
    elapsed = 0.0
    if x0 is not None:
        t0 = time.perf_counter()
        if method in _TAKES_X0_Y0:                                              # krylov_solve!(ws, A, b, c, x0, y0; kwargs...)
            ws.warm_start_(x0, full.pop("y0", None))
        else:
            ws.warm_start_(x0)
        elapsed = time.perf_counter() - t0
        full["timemax"] = full["timemax"] - elapsed
    inplace(ws, A, b, **full)
    ws._timer_extra = elapsed
    return ws


def krylov_solve(method: str, A, b, x0=None, ctx: Context | None = None, **kw):
    """krylov_solve(Val(method), A, b[, x0]; kwargs...) = method(A, b[, x0]; kwargs...) (src/interface.jl:146-199): a fresh
    workspace (its creation charged to `timemax` and `stats.timer`), every keyword forwarded.  Returns (x, stats, workspace)."""
    wkw = {k: kw.pop(k) for k in list(kw) if k in _workspace_kwargs(method)}
    t0 = time.perf_counter()
    if method == "cg_lanczos_shift":                     # krylov_solve(Val(:cg_lanczos_shift), A, b, shifts; kwargs...)
        shifts = np.asarray(x0 if x0 is not None else kw.pop("shifts"), dtype=np.float64)
        ws = krylov_workspace(method, A, b, len(shifts), **wkw)
        elapsed = time.perf_counter() - t0
        full = _forward(method, kw)
        full["timemax"] = full["timemax"] - elapsed
        cg_lanczos_shift_(ws, A, b, shifts, **full)
        ws._timer_extra = elapsed
        return ws.x, ws.stats, ws
    if method == "block_gmres":
        B = np.asarray(b, dtype=np.float64)
        ctx = ctx or A.ctx
        ws = krylov_workspace(method, A, B, ctx=ctx, **wkw)
        b = ctx.array(np.asfortranarray(B).ravel(order="F"))
    elif method in _TAKES_C:                           # krylov_solve(Val(:usymqr), A, b, c[, x0]; kwargs...): c travels as a keyword here
        if kw.get("c") is None:
            raise KhipError(-1, f"{method}: c (the starting vector of the second Krylov space) is required")
        ws = krylov_workspace(method, A, b, kw["c"], **wkw)
    else:
        ws = krylov_workspace(method, A, b, **wkw)
    if x0 is not None:
        if method in _TAKES_X0_Y0:
            ws.warm_start_(x0, kw.pop("y0", None))
        else:
            ws.warm_start_(x0)
    elapsed = time.perf_counter() - t0
    full = _forward(method, kw)
    full["timemax"] = full["timemax"] - elapsed
    _INPLACE[type(ws)][1](ws, A, b, **full)
    ws._timer_extra = elapsed
    if method in _TAKES_X0_Y0:
        return ws.x, ws.y, ws.stats, ws
    return (ws.X if method == "block_gmres" else ws.x), ws.stats, ws


def cg(A, b: DeviceVector, x0=None, **kw):
    """Out-of-place cg(A, b[, x0]; kwargs...) -> (x, stats, workspace) (src/interface.jl:146-154, 160-170)."""
    return krylov_solve("cg", A, b, x0, **kw)


def gmres(A, b: DeviceVector, x0=None, **kw):
    return krylov_solve("gmres", A, b, x0, **kw)


def bicgstab(A, b: DeviceVector, x0=None, **kw):
    return krylov_solve("bicgstab", A, b, x0, **kw)


def minres(A, b: DeviceVector, x0=None, **kw):
    """Out-of-place minres(A, b[, x0]; window, kwargs...) -> (x, stats, workspace) (src/minres.jl:164-172)."""
    return krylov_solve("minres", A, b, x0, **kw)


def bilq(A, b: DeviceVector, x0=None, **kw):
    """Out-of-place bilq(A, b[, x0]; kwargs...) -> (x, stats, workspace) (src/bilq.jl:118-126); A' is taken once and kept on A."""
    return krylov_solve("bilq", A, b, x0, **kw)


def qmr(A, b: DeviceVector, x0=None, **kw):
    """Out-of-place qmr(A, b[, x0]; kwargs...) -> (x, stats, workspace) (src/qmr.jl:124-132); A' is taken once and kept on A."""
    return krylov_solve("qmr", A, b, x0, **kw)


def usymqr(A, b: DeviceVector, c: DeviceVector, x0=None, **kw):
    """Out-of-place usymqr(A, b, c[, x0]; kwargs...) -> (x, stats, workspace) (src/usymqr.jl:16-23); A' is taken once and kept on A."""
    return krylov_solve("usymqr", A, b, x0, c=c, **kw)


def usymlq(A, b: DeviceVector, c: DeviceVector, x0=None, **kw):
    """Out-of-place usymlq(A, b, c[, x0]; kwargs...) -> (x, stats, workspace) (src/usymlq.jl:16-24); A' is taken once and kept on A."""
    return krylov_solve("usymlq", A, b, x0, c=c, **kw)


def cgs(A, b: DeviceVector, x0=None, **kw):
    """Out-of-place cgs(A, b[, x0]; kwargs...) -> (x, stats, workspace) (src/cgs.jl:126-134)."""
    return krylov_solve("cgs", A, b, x0, **kw)


def symmlq(A, b: DeviceVector, x0=None, **kw):
    """Out-of-place symmlq(A, b[, x0]; window, kwargs...) -> (x, stats, workspace) (src/symmlq.jl:16-22)."""
    return krylov_solve("symmlq", A, b, x0, **kw)


def minres_qlp(A, b: DeviceVector, x0=None, **kw):
    """Out-of-place minres_qlp(A, b[, x0]; kwargs...) -> (x, stats, workspace) (src/minres_qlp.jl:20-26)."""
    return krylov_solve("minres_qlp", A, b, x0, **kw)


def _solve_pair(method: str, WsClass, A, b, c, x0, y0, kw):
    """Out-of-place method(A, b, c[, x0, y0]; kwargs...) -> (x, y, stats, workspace) of the solvers with two solutions.  The
    workspace's creation and the warm start are charged to `timemax` and `stats.timer`, as krylov_solve does."""
    wkw = {k: kw.pop(k) for k in list(kw) if k in ("adopt", "vectors")}
    t0 = time.perf_counter()
    n = len(c) if issubclass(WsClass, _TwoSidedWorkspace) else len(b)           # bilqr! is square
    ws = WsClass(b.ctx, len(b), n, **wkw)
    if x0 is not None or y0 is not None:
        ws.warm_start_(x0, y0)
    elapsed = time.perf_counter() - t0
    full = _forward(method, kw)
    full["timemax"] = full["timemax"] - elapsed
    _INPLACE[WsClass][1](ws, A, b, c, **full)
    ws._timer_extra = elapsed
    return ws.x, ws.y, ws.stats, ws


def bilqr(A, b: DeviceVector, c: DeviceVector, x0=None, y0=None, **kw):
    """Out-of-place bilqr(A, b, c[, x0, y0]; kwargs...) -> (x, y, stats, workspace) (src/bilqr.jl:16-26); A' is taken once and kept
    on A.  The workspace's creation and the warm start are charged to `timemax` and `stats.timer`, as krylov_solve does."""
    return _solve_pair("bilqr", BilqrWorkspace, A, b, c, x0, y0, kw)


def trilqr(A, b: DeviceVector, c: DeviceVector, x0=None, y0=None, **kw):
    """Out-of-place trilqr(A, b, c[, x0, y0]; kwargs...) -> (x, t, stats, workspace) (src/trilqr.jl:16-26); A' is taken once and kept
    on A.  The workspace's creation and the warm start are charged to `timemax` and `stats.timer`, as krylov_solve does."""
    return _solve_pair("trilqr", TrilqrWorkspace, A, b, c, x0, y0, kw)


def tricg(A, b: DeviceVector, c: DeviceVector, x0=None, y0=None, **kw):
    """Out-of-place tricg(A, b, c[, x0, y0]; kwargs...) -> (x, y, stats, workspace) (src/tricg.jl:16-33); A' is taken once and kept on
    A.  The workspace's creation and the warm start are charged to `timemax` and `stats.timer`, as krylov_solve does."""
    return _solve_pair("tricg", TricgWorkspace, A, b, c, x0, y0, kw)


def trimr(A, b: DeviceVector, c: DeviceVector, x0=None, y0=None, **kw):
    """Out-of-place trimr(A, b, c[, x0, y0]; kwargs...) -> (x, y, stats, workspace) (src/trimr.jl:16-34); A' is taken once and kept on
    A.  The workspace's creation and the warm start are charged to `timemax` and `stats.timer`, as krylov_solve does."""
    return _solve_pair("trimr", TrimrWorkspace, A, b, c, x0, y0, kw)


def usymlqr(A, b: DeviceVector, c: DeviceVector, x0=None, y0=None, **kw):
    """Out-of-place usymlqr(A, b, c[, x0, y0]; kwargs...) -> (x, y, stats, workspace) (src/usymlqr.jl:20-32); A' is taken once and kept
    on A.  The workspace's creation and the warm start are charged to `timemax` and `stats.timer`, as krylov_solve does."""
    return _solve_pair("usymlqr", UsymlqrWorkspace, A, b, c, x0, y0, kw)


def cg_lanczos_shift(A, b: DeviceVector, shifts, **kw):
    """Out-of-place cg_lanczos_shift(A, b, shifts; kwargs...) -> (x, stats, workspace), x a list of one DeviceVector per shift."""
    return krylov_solve("cg_lanczos_shift", A, b, shifts, **kw)


# --------------------------------------------------------------------------- Krylov processes
# src/krylov_processes.jl: same names, arguments and return values; the bases live in HBM.

class DeviceMatrix:
    """Dense column-major n x ncols Float64 matrix in HBM (`M(undef, n, k+1)`, src/krylov_processes.jl:52):
    column j is the DeviceVector `col(j)`; the leading dimension is n rounded up to 32 doubles."""

    def __init__(self, ctx: Context, n: int, ncols: int):
        self.ctx, self.n, self.ncols = ctx, int(n), int(ncols)
        self.ld = max(32, (self.n + 31) & ~31)
        self.buf = DeviceVector(ctx, self.ld * self.ncols)

    @property
    def ptr(self):
        return self.buf.ptr

    @property
    def shape(self):
        return (self.n, self.ncols)

    def col(self, j: int) -> DeviceVector:
        return self.buf.slice(j * self.ld, j * self.ld + self.n)

    def to_host(self) -> np.ndarray:
        return np.asfortranarray(self.buf.to_host().reshape(self.ncols, self.ld)[:, :self.n].T)


def _tridiag_from_nzval(k, nz):
    """The (k+1) x k SparseMatrixCSC of src/krylov_processes.jl:35-48 as scipy CSC."""
    import scipy.sparse as sp
    colptr = np.zeros(k + 1, dtype=np.int64)
    rowval = np.zeros(3 * k - 1, dtype=np.int64)
    for i in range(1, k + 1):
        pos = colptr[i - 1]
        colptr[i] = 3 * i - 1
        if i == 1:
            rowval[pos], rowval[pos + 1] = 0, 1
        else:
            rowval[pos], rowval[pos + 1], rowval[pos + 2] = i - 2, i - 1, i
    return sp.csc_matrix((nz, rowval, colptr), shape=(k + 1, k))


def _bidiag_from_nzval(k, nz):
    """The (k+1) x (k+1) lower bidiagonal SparseMatrixCSC of src/krylov_processes.jl:331-347 as scipy CSC."""
    import scipy.sparse as sp
    colptr = np.zeros(k + 2, dtype=np.int64)
    rowval = np.zeros(2 * k + 1, dtype=np.int64)
    for i in range(1, k + 2):
        pos = colptr[i - 1]
        if i <= k:
            colptr[i] = pos + 2
            rowval[pos], rowval[pos + 1] = i - 1, i
        else:
            colptr[i] = pos + 1
            rowval[pos] = i - 1
    return sp.csc_matrix((nz, rowval, colptr), shape=(k + 1, k + 1))


def _basis(ctx, n, ncols, out):
    if out is None:
        return DeviceMatrix(ctx, n, ncols)
    if out.shape != (n, ncols):
        raise ValueError(f"basis storage is {out.shape}, need {(n, ncols)}")
    return out


def hermitian_lanczos(A, b: DeviceVector, k: int, allow_breakdown=False, reorthogonalization=False, V=None):
    """V, beta1, T = hermitian_lanczos(A, b, k; allow_breakdown, reorthogonalization) (src/krylov_processes.jl:28-102).
    V: DeviceMatrix n x (k+1) (pass `V=` to reuse storage); T: scipy CSC (k+1) x k."""
    ctx, n, keep = b.ctx, len(b), []
    V = _basis(ctx, n, k + 1, V)
    beta, nz = C.c_double(), np.zeros(3 * k - 1)
    _ck(lib().khip_hermitian_lanczos(ctx._h, _make_operator(ctx, A, n, keep), n, b.ptr, k, int(allow_breakdown),
                                     int(reorthogonalization), V.ptr, V.ld, C.byref(beta), nz.ctypes.data_as(c_double_p)))
    return V, beta.value, _tridiag_from_nzval(k, nz)


def arnoldi(A, b: DeviceVector, k: int, allow_breakdown=False, reorthogonalization=False, V=None):
    """V, beta, H = arnoldi(A, b, k; allow_breakdown, reorthogonalization) (src/krylov_processes.jl:250-296).
    V: DeviceMatrix n x (k+1) (pass `V=` to reuse storage); H: dense (k+1) x k numpy array."""
    ctx, n, keep = b.ctx, len(b), []
    V = _basis(ctx, n, k + 1, V)
    beta, H = C.c_double(), np.zeros((k + 1, k), order="F")
    _ck(lib().khip_arnoldi(ctx._h, _make_operator(ctx, A, n, keep), n, b.ptr, k, int(allow_breakdown),
                           int(reorthogonalization), V.ptr, V.ld, C.byref(beta), H.ctypes.data_as(c_double_p)))
    return V, beta.value, H


def golub_kahan(A, b: DeviceVector, k: int, allow_breakdown=False, At=None, n=None, V=None, U=None):
    """V, U, beta1, L = golub_kahan(A, b, k; allow_breakdown) (src/krylov_processes.jl:323-398).  A: CsrMatrix (its
    adjoint is built with A.transpose() unless `At` is given) or a callable together with a callable `At` and the
    column count `n` (`size(A, 2)`)."""
    ctx, m, keep = b.ctx, len(b), []
    if At is None:
        if not isinstance(A, CsrMatrix):
            raise TypeError("golub_kahan: a callable A needs the adjoint callable At")
        At = A.transpose()
    if isinstance(A, CsrMatrix):
        n = A.n
    elif n is None:
        raise TypeError("golub_kahan: a callable A needs n = size(A, 2)")
    V, U = _basis(ctx, n, k + 1, V), _basis(ctx, m, k + 1, U)
    beta, nz = C.c_double(), np.zeros(2 * k + 1)
    # callbacks receive (x, y) sized for their own direction
    opA = _make_operator(ctx, A, n, keep) if isinstance(A, CsrMatrix) else _make_operator_mn(ctx, A, n, m, keep)
    opAt = _make_operator(ctx, At, m, keep) if isinstance(At, CsrMatrix) else _make_operator_mn(ctx, At, m, n, keep)
    _ck(lib().khip_golub_kahan(ctx._h, opA, opAt, m, n, b.ptr, k, int(allow_breakdown), V.ptr, V.ld, U.ptr, U.ld,
                               C.byref(beta), nz.ctypes.data_as(c_double_p)))
    return V, U, beta.value, _bidiag_from_nzval(k, nz)


def _op_mn(ctx, op, nin, nout, keep):
    return _make_operator(ctx, op, nin, keep) if isinstance(op, CsrMatrix) else _make_operator_mn(ctx, op, nin, nout, keep)


def nonhermitian_lanczos(A, b: DeviceVector, c: DeviceVector, k: int, allow_breakdown=False, At=None, V=None, U=None):
    """V, beta1, T, U, gamma1, Tt = nonhermitian_lanczos(A, b, c, k; allow_breakdown) (src/krylov_processes.jl:133-222)."""
    ctx, n, keep = b.ctx, len(b), []
    if At is None:
        if not isinstance(A, CsrMatrix):
            raise TypeError("nonhermitian_lanczos: a callable A needs the adjoint callable At")
        At = A.transpose()
    V, U = _basis(ctx, n, k + 1, V), _basis(ctx, n, k + 1, U)
    beta, gamma, nt, nh = C.c_double(), C.c_double(), np.zeros(3 * k - 1), np.zeros(3 * k - 1)
    _ck(lib().khip_nonhermitian_lanczos(ctx._h, _op_mn(ctx, A, n, n, keep), _op_mn(ctx, At, n, n, keep), n, b.ptr, c.ptr, k,
                                        int(allow_breakdown), V.ptr, V.ld, U.ptr, U.ld, C.byref(beta), C.byref(gamma),
                                        nt.ctypes.data_as(c_double_p), nh.ctypes.data_as(c_double_p)))
    return V, beta.value, _tridiag_from_nzval(k, nt), U, gamma.value, _tridiag_from_nzval(k, nh)


def saunders_simon_yip(A, b: DeviceVector, c: DeviceVector, k: int, allow_breakdown=False, At=None, V=None, U=None):
    """V, beta1, T, U, gamma1, Tt = saunders_simon_yip(A, b, c, k; allow_breakdown) (src/krylov_processes.jl:431-524).
    A is m x n, b has length m, c has length n."""
    ctx, m, n, keep = b.ctx, len(b), len(c), []
    if At is None:
        if not isinstance(A, CsrMatrix):
            raise TypeError("saunders_simon_yip: a callable A needs the adjoint callable At")
        At = A.transpose()
    V, U = _basis(ctx, m, k + 1, V), _basis(ctx, n, k + 1, U)
    beta, gamma, nt, nh = C.c_double(), C.c_double(), np.zeros(3 * k - 1), np.zeros(3 * k - 1)
    _ck(lib().khip_saunders_simon_yip(ctx._h, _op_mn(ctx, A, n, m, keep), _op_mn(ctx, At, m, n, keep), m, n, b.ptr, c.ptr, k,
                                      int(allow_breakdown), V.ptr, V.ld, U.ptr, U.ld, C.byref(beta), C.byref(gamma),
                                      nt.ctypes.data_as(c_double_p), nh.ctypes.data_as(c_double_p)))
    return V, beta.value, _tridiag_from_nzval(k, nt), U, gamma.value, _tridiag_from_nzval(k, nh)


def montoison_orban(A, B, b: DeviceVector, c: DeviceVector, k: int, allow_breakdown=False, reorthogonalization=False,
                    V=None, U=None):
    """V, beta, H, U, gamma, F = montoison_orban(A, B, b, c, k; allow_breakdown, reorthogonalization)
    (src/krylov_processes.jl:553-632).  A is m x n, B is n x m, b has length m, c has length n."""
    ctx, m, n, keep = b.ctx, len(b), len(c), []
    V, U = _basis(ctx, m, k + 1, V), _basis(ctx, n, k + 1, U)
    beta, gamma = C.c_double(), C.c_double()
    H, F = np.zeros((k + 1, k), order="F"), np.zeros((k + 1, k), order="F")
    _ck(lib().khip_montoison_orban(ctx._h, _op_mn(ctx, A, n, m, keep), _op_mn(ctx, B, m, n, keep), m, n, b.ptr, c.ptr, k,
                                   int(allow_breakdown), int(reorthogonalization), V.ptr, V.ld, U.ptr, U.ld,
                                   C.byref(beta), C.byref(gamma), H.ctypes.data_as(c_double_p), F.ctypes.data_as(c_double_p)))
    return V, beta.value, H, U, gamma.value, F


def _make_operator_mn(ctx, op, nin, nout, keep):
    """callable(x: DeviceVector[nin], y: DeviceVector[nout]) -> POINTER(COperator) for rectangular operators."""
    def thunk(_self, xp, yp):
        try:
            op(DeviceVector(ctx, nin, ptr=xp), DeviceVector(ctx, nout, ptr=yp))
            return 0
        except Exception as e:
            sys.stderr.write(f"operator callback failed: {e}\n")
            return 1
    fn = APPLY_FN(thunk)
    co = COperator()
    co.csr, co.apply = None, fn
    keep.extend([fn, co])
    return C.byref(co)


# --------------------------------------------------------------------------- host-only partition helpers

def row_partition(n: int, nranks: int):
    """Contiguous 1-D row partition: rank g owns rows [g*n//G, (g+1)*n//G)."""
    return [(g * n) // nranks for g in range(nranks + 1)]


def ghost_columns_host(rowptr, col, row0):
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
    col = np.ascontiguousarray(col, dtype=np.int32)
    m = rowptr.size - 1
    cnt = C.c_int64()
    out = np.empty(max(col.size, 1), dtype=np.int32)
    _ck(lib().khip_ghost_columns_host(rowptr.ctypes.data, col.ctypes.data, m, row0, out.ctypes.data, out.size,
                                      C.byref(cnt)))
    return out[: cnt.value].copy()


def halo_plan_host(rank, nranks, row_starts, ghost_lists):
    row_starts = np.ascontiguousarray(row_starts, dtype=np.int64)
    off = np.zeros(nranks + 1, dtype=np.int64)
    for r in range(nranks):
        off[r + 1] = off[r] + len(ghost_lists[r])
    allg = np.ascontiguousarray(np.concatenate([np.asarray(g, dtype=np.int32) for g in ghost_lists])
                                if off[-1] else np.zeros(1, dtype=np.int32), dtype=np.int32)
    recv_off = np.zeros(nranks + 1, dtype=np.int64)
    send_off = np.zeros(nranks + 1, dtype=np.int64)
    cap = int(off[-1]) + 1
    send_idx = np.zeros(cap, dtype=np.int32)
    _ck(lib().khip_halo_plan_host(rank, nranks, row_starts.ctypes.data, allg.ctypes.data, off.ctypes.data,
                                  recv_off.ctypes.data, send_off.ctypes.data, send_idx.ctypes.data, cap))
    return recv_off, send_off, send_idx[: send_off[-1]].copy()


# --------------------------------------------------------------------------- block-GMRES (panels)

def panel_rows(n: int) -> int:
    out = C.c_int64()
    _ck(lib().khip_panel_rows(n, C.byref(out)))
    return out.value


class Panel:
    """n x p block in HBM, ROW-MAJOR with the row count padded to 16 (csrc/panel.hip).  The reference's
    `SM(undef, n, p)` storage (src/block_krylov_workspaces.jl:137-163) in the layout the MFMA kernels want."""

    def __init__(self, ctx: Context, n: int, p: int):
        self.ctx, self.n, self.p = ctx, n, p
        self.n_pad = panel_rows(n)
        self.buf = ctx.zeros(self.n_pad * p)

    @classmethod
    def from_host(cls, ctx, M):
        M = np.asarray(M, dtype=np.float64)
        P = cls(ctx, M.shape[0], M.shape[1])
        col = ctx.array(np.asfortranarray(M).ravel(order="F"))
        _ck(lib().khip_panel_from_colmajor(ctx._h, P.n, P.p, col.ptr, P.buf.ptr))
        ctx.sync()
        return P

    @classmethod
    def from_raw_buffer(cls, ctx, n, buf):
        """A panel of n rows whose WHOLE row-major buffer, padding rows included, is the host array buf (panel_rows(n) x p):
        for tests that place values in the padding rows and read `buf` back raw."""
        buf = np.ascontiguousarray(buf, dtype=np.float64)
        if buf.ndim != 2 or buf.shape[0] != panel_rows(n):
            raise ValueError(f"from_raw_buffer: {buf.shape} is not ({panel_rows(n)}, p) for n = {n}")
        P = cls.__new__(cls)
        P.ctx, P.n, P.p, P.n_pad = ctx, n, buf.shape[1], buf.shape[0]
        P.buf = ctx.array(buf.ravel())
        return P

    def to_host(self) -> np.ndarray:
        col = self.ctx.empty(self.n * self.p)
        _ck(lib().khip_panel_to_colmajor(self.ctx._h, self.n, self.p, self.buf.ptr, col.ptr))
        return col.to_host().reshape(self.p, self.n).T.copy()


def panel_gemm_tn(V: Panel, Q: Panel) -> np.ndarray:
    """Psi = V' * Q  (mul!(R, V', Q), src/block_gmres.jl:245)."""
    out = np.zeros((V.p, V.p), order="F")
    _ck(lib().khip_panel_gemm_tn(V.ctx._h, V.n, V.p, V.buf.ptr, Q.buf.ptr, out.ctypes.data_as(c_double_p)))
    return out


def panel_gemm_nn_(alpha, V: Panel, Psi, beta, Q: Panel) -> Panel:
    """Q = beta Q + alpha V Psi  (mul!(Q, V, Psi, alpha, beta), src/block_gmres.jl:246)."""
    Pf = np.asfortranarray(Psi, dtype=np.float64)
    _ck(lib().khip_panel_gemm_nn(V.ctx._h, V.n, V.p, alpha, V.buf.ptr, Pf.ctypes.data_as(c_double_p), beta, Q.buf.ptr))
    return Q


def panel_mgs_(V, Q: Panel, accumulate_into=None):
    """Block Gram-Schmidt sweep of Q against the panels V[0..k) (src/block_gmres.jl:244-247) -> list of k p x p blocks."""
    k, p = len(V), Q.p
    ptrs = (C.c_void_p * max(k, 1))(*[v.buf.ptr for v in V])
    out = np.zeros((k, p * p)) if accumulate_into is None else np.ascontiguousarray(
        np.stack([np.asarray(b, dtype=np.float64).ravel(order="F") for b in accumulate_into]))
    _ck(lib().khip_panel_mgs(Q.ctx._h, Q.n, p, k, ptrs, Q.buf.ptr, out.ctypes.data_as(c_double_p),
                             0 if accumulate_into is None else 1))
    return [out[i].reshape(p, p, order="F").copy() for i in range(k)]


def panel_qr_(Q: Panel) -> np.ndarray:
    """Reduced QR in place (householder!(Q, R, tau), src/block_krylov_utils.jl:201-208); returns R."""
    R = np.zeros((Q.p, Q.p), order="F")
    _ck(lib().khip_panel_qr(Q.ctx._h, Q.n, Q.p, Q.buf.ptr, R.ctypes.data_as(c_double_p)))
    return R


def panel_multi_nn_(Vs, Ys, beta: float, X: Panel) -> Panel:
    """X <- beta X + sum_i V_i Y_i in the order i = 0..k-1 (src/block_gmres.jl:324-326 in one pass); Ys: k host p x p blocks."""
    k = len(Vs)
    ptrs = (C.c_void_p * max(k, 1))(*[v.buf.ptr for v in Vs])
    Y = np.ascontiguousarray(np.concatenate([np.asfortranarray(y, dtype=np.float64).ravel(order="F") for y in Ys])) if k else np.zeros(1)
    _ck(lib().khip_panel_multi_nn(X.ctx._h, X.n, X.p, k, ptrs, Y.ctypes.data_as(c_double_p), float(beta), X.buf.ptr))
    return X


def panel_qr_tau_(Q: Panel):
    """householder!(Q, R, tau): Q, R and tau as kgeqrf! + korgqr! leave them (LAPACK signs); returns (R, tau)."""
    R = np.zeros((Q.p, Q.p), order="F")
    tau = np.zeros(Q.p)
    _ck(lib().khip_panel_qr_tau(Q.ctx._h, Q.n, Q.p, Q.buf.ptr, R.ctypes.data_as(c_double_p), tau.ctypes.data_as(c_double_p)))
    return R, tau


def panel_norm(Q: Panel) -> float:
    r = C.c_double()
    _ck(lib().khip_panel_norm(Q.ctx._h, Q.n, Q.p, Q.buf.ptr, C.byref(r)))
    return r.value


def spmm_(A: CsrMatrix, X: Panel, Y: Panel) -> Panel:
    _ck(lib().khip_spmm(A.ctx._h, A._h, X.buf.ptr, Y.buf.ptr, X.p))
    return Y


class BlockGmresWorkspace(_Workspace):
    """BlockGmresWorkspace(m, n, p, SV, SM; memory = 5) (src/block_krylov_workspaces.jl:115-171).  Adopted form: the tall
    blocks X, W, V[i] are Panels of this side (the HIPMatrix of julia/KrylovHIP), the small blocks live in the library."""
    _prefix = "block_gmres"

    def __init__(self, ctx: Context, m: int, n: int, p: int, memory: int = 5, adopt: bool | None = None):
        self.ctx, self.m, self.n, self.p, self.memory = ctx, m, n, p, memory
        self.adopted = _adopt_default() if adopt is None else bool(adopt)
        self._h = C.c_void_p()
        if self.adopted:
            mem = 5 if memory <= 0 else memory
            mem = max(1, min(n // p, mem))                                     # memory = min(div(n, p), memory), :138
            t0 = time.perf_counter()
            self._pan = {k: Panel(ctx, n, p) for k in ("X", "W")}
            self.V = [Panel(ctx, n, p) for _ in range(mem)]
            self._alloc_s = time.perf_counter() - t0
            ptrs = (C.c_void_p * mem)(*[v.buf.ptr for v in self.V])
            _ck(lib().khip_block_gmres_workspace_adopt(ctx._h, m, n, p, mem, self._pan["X"].buf.ptr, self._pan["W"].buf.ptr, ptrs,
                                                       C.byref(self._h)))

            def grow(_ud):                                                     # push!(V, SM(undef, n, p)), src/block_gmres.jl:300-305
                try:
                    self.V.append(Panel(self.ctx, self.n, self.p))
                    return self.V[-1].buf.ptr
                except Exception as e:
                    sys.stderr.write(f"grow callback failed: {e}\n")
                    return None
            self._grow = GROW_FN(grow)
            _ck(lib().khip_block_gmres_workspace_set_grow(self._h, self._grow, None))
        else:
            _ck(lib().khip_block_gmres_workspace_create(ctx._h, m, n, p, memory, C.byref(self._h)))

    def _allocate_panel_if(self, cond: bool, name: str):
        if cond and self.adopted and name not in self._pan:
            t0 = time.perf_counter()
            P = Panel(self.ctx, self.n, self.p)
            self._alloc_s += time.perf_counter() - t0
            self._pan[name] = P
            _ck(lib().khip_block_gmres_workspace_adopt_panel(self._h, name.encode(), P.buf.ptr))

    @property
    def X(self) -> np.ndarray:
        if self.adopted:
            return self._pan["X"].to_host()
        col = self.ctx.empty(self.n * self.p)
        _ck(lib().khip_block_gmres_get_X(self._h, col.ptr))
        return col.to_host().reshape(self.p, self.n).T.copy()

    x = X

    def warm_start_(self, X0):
        if self.adopted:                                                       # allocate_if(true, ws, :ΔX, ...); copyto!(ws.ΔX, X0)
            self._allocate_panel_if(True, "dX")
            P0 = Panel.from_host(self.ctx, np.asarray(X0, dtype=np.float64))
            kcopy_(P0.n_pad * P0.p, self._pan["dX"].buf, P0.buf)
            _ck(lib().khip_block_gmres_warm_start_panel(self._h, self._pan["dX"].buf.ptr))
            return self
        col = self.ctx.array(np.asfortranarray(np.asarray(X0, dtype=np.float64)).ravel(order="F"))
        _ck(lib().khip_block_gmres_warm_start(self._h, col.ptr))
        return self

    @property
    def nbytes(self):
        """Workspace bytes as test/test_allocations.jl:734-761 counts them (includes `nbytes_extra`)."""
        return lib().khip_block_gmres_workspace_bytes(self._h, None)

    @property
    def nbytes_extra(self):
        e = C.c_size_t()
        lib().khip_block_gmres_workspace_bytes(self._h, C.byref(e))
        return e.value


def _make_block_operator(ctx, op, n, p, keep):
    """CsrMatrix | callable(X: Panel, Y: Panel) | None for the block solver (callbacks see row-major panels)."""
    if op is None or isinstance(op, CsrMatrix):
        return _make_operator(ctx, op, n, keep)

    def thunk(_self, xp, yp):
        try:
            X, Y = Panel.__new__(Panel), Panel.__new__(Panel)
            for P_, ptr in ((X, xp), (Y, yp)):
                P_.ctx, P_.n, P_.p, P_.n_pad = ctx, n, p, panel_rows(n)
                P_.buf = DeviceVector(ctx, P_.n_pad * p, ptr=ptr)
            op(X, Y)
            return 0
        except Exception as e:
            sys.stderr.write(f"block operator callback failed: {e}\n")
            return 1
    fn = APPLY_FN(thunk)
    co = COperator()
    co.csr, co.apply = None, fn
    keep.extend([fn, co])
    return C.byref(co)


def block_gmres_(ws: BlockGmresWorkspace, A, B_colmajor: DeviceVector, M=None, N=None, **kw):
    """block_gmres!(workspace, A, B; restart, reorthogonalization, atol, rtol, itmax, history, ...)
    (src/block_gmres.jl:110-358); B is an n x p column-major device array."""
    keep = []
    opts = _make_options(keep=keep, ws=ws, **kw)
    ops = (_make_block_operator(ws.ctx, A, ws.n, ws.p, keep), _make_block_operator(ws.ctx, M, ws.n, ws.p, keep),
           _make_block_operator(ws.ctx, N, ws.n, ws.p, keep))
    if ws.adopted:
        # the binding's matrix type IS a panel (HIPMatrix(B::Matrix) converts once, at construction): B is read in place
        ws._allocate_panel_if(M is not None, "Q")                                          # src/block_gmres.jl:146-147
        ws._allocate_panel_if(N is not None, "P")
        ws._allocate_panel_if(bool(kw.get("restart")), "dX")
        if isinstance(B_colmajor, Panel):
            Bp = B_colmajor
        else:
            Bp = Panel(ws.ctx, ws.n, ws.p)
            _ck(lib().khip_panel_from_colmajor(ws.ctx._h, ws.n, ws.p, _p(B_colmajor), Bp.buf.ptr))
        keep.append(Bp)
        rc = lib().khip_block_gmres_solve_panel(ws._h, *ops, Bp.buf.ptr, C.byref(opts))
    else:
        if isinstance(B_colmajor, Panel):            # a library-owned workspace takes B column-major (khip_block_gmres_solve)
            col = ws.ctx.empty(ws.n * ws.p)
            _ck(lib().khip_panel_to_colmajor(ws.ctx._h, ws.n, ws.p, B_colmajor.buf.ptr, col.ptr))
            keep.append(col)
            B_colmajor = col
        rc = lib().khip_block_gmres_solve(ws._h, *ops, _p(B_colmajor), C.byref(opts))
    return _finish(ws, rc)


def block_gmres(A, B, X0=None, ctx=None, **kw):
    """Out-of-place block_gmres(A, B[, X0]; memory, kwargs...) for a host n x p array B -> (X, stats, workspace)
    (src/interface.jl:247-290)."""
    return krylov_solve("block_gmres", A, B, X0, ctx=ctx, **kw)


_INPLACE.update({CgWorkspace: ("cg", cg_), GmresWorkspace: ("gmres", gmres_), BicgstabWorkspace: ("bicgstab", bicgstab_),
                 BlockGmresWorkspace: ("block_gmres", block_gmres_), MinresWorkspace: ("minres", minres_), BilqWorkspace: ("bilq", bilq_),
                 QmrWorkspace: ("qmr", qmr_), CgsWorkspace: ("cgs", cgs_), UsymqrWorkspace: ("usymqr", usymqr_),
                 UsymlqWorkspace: ("usymlq", usymlq_),
                 TrilqrWorkspace: ("trilqr", trilqr_),
                 TricgWorkspace: ("tricg", tricg_),
                 TrimrWorkspace: ("trimr", trimr_),
                 UsymlqrWorkspace: ("usymlqr", usymlqr_),
                 SymmlqWorkspace: ("symmlq", symmlq_),
                 MinresQlpWorkspace: ("minres_qlp", minres_qlp_),
                 BilqrWorkspace: ("bilqr", bilqr_),
                 CgLanczosShiftWorkspace: ("cg_lanczos_shift", cg_lanczos_shift_)})
