"""navierstokes_amd.mpk — host-side mirror of the reference's mpk/ interface.

Same names, argument order and meaning as the free functions of the
reference's ``mpk/SpMV.h:52-66`` (plus the per-file kernels ``SpM2V_CSR``
``mpk/SpM2V.cpp:80``, ``SpM4V`` ``mpk/SpMVmulti0.cpp:191`` and
``orthogonalize`` ``mpk/SpMVmulti.cpp:146``), so that tests read like the
reference's harnesses: ``SpMV_CSR(y, x, A)`` overwrites ``y`` with ``A x``.

Everything is computed by the HIP library ``csrc/libmi355spmv.so`` through its
C-ABI (``include/mi355_spmv.h``).  PyTorch appears only as plumbing: vectors
may be CUDA/HIP tensors (device-resident, launched on torch's current stream,
no synchronisation) or numpy arrays (copied in and out like the reference's
CPU functions).  There is NO CPU fallback: importing this module without the
built library, or calling it without a GPU, raises.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MI355_SPMV_LIBRARY") or os.path.join(_HERE, "csrc", "libmi355spmv.so")  # env: A/B of two builds (tools/)

MI_OK = 0
KERNEL_AUTO, KERNEL_STREAM, KERNEL_RING, KERNEL_ROWPAR = 0, 1, 2, 3
KERNELS = {"auto": 0, "stream": 1, "ring": 2, "rowpar": 3, "bcsr4": 4, "tile": 5, "mring": 6, "sstream": 7}

_c = ctypes
_vp = ctypes.c_void_p
_LIB = None


class MiError(RuntimeError):
    def __init__(self, status, detail):
        super().__init__(f"libmi355spmv status {status}: {detail}")
        self.status = status


def lib():
    """The loaded C-ABI library (loads torch's HIP runtime first when torch is around)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing — the HIP extension was not built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). "
            "There is no CPU fallback for this path."
        )
    try:  # one HIP runtime per process: let torch's copy win if torch is installed
        import torch  # noqa: F401
    except Exception:
        pass
    L = ctypes.CDLL(LIB_PATH)
    L.mi_strerror.restype = _c.c_char_p
    L.mi_last_error.restype = _c.c_char_p
    L.mi_csr_kernel_name.restype = _c.c_char_p
    L.mi_csr_kernel_name.argtypes = [_vp]
    i, ll, d = _c.c_int, _c.c_longlong, _c.c_double
    P = _c.POINTER
    sigs = {
        "mi_version": [],
        "mi_device_count": [P(i)],
        "mi_set_device": [i],
        "mi_device_synchronize": [],
        "mi_flush_cache": [],
        "mi_flush_cache_async": [_vp],
        "mi_csr_create": [i, i, _vp, _vp, _vp, P(_vp)],
        "mi_csr_create_mapped": [i, i, _vp, _vp, _vp, _vp, P(_vp)],
        "mi_csr_destroy": [_vp],
        "mi_csr_update_values": [_vp, _vp],
        "mi_csr_update_values_dev": [_vp, _vp, _vp],
        "mi_bcsr4_update_values": [_vp, _vp],
        "mi_bcsr4_update_values_dev": [_vp, _vp, _vp],
        "mi_orthonormalize_against_basis": [i, i, _vp, _vp, _vp],
        "mi_orthonormalize_against_basis_dev": [i, i, _vp, _vp, _vp, _vp],
        "mi_mdot": [i, i, _vp, _vp, _vp],
        "mi_mdot_dev": [i, i, _vp, _vp, _vp, _vp],
        "mi_maxpy": [i, i, _vp, i, _vp, _vp],
        "mi_maxpy_dev": [i, i, _vp, i, _vp, _vp, _vp, _vp],
        "mi_cgs_dev": [i, i, _vp, _vp, i, _vp, _vp, _vp],
        "mi_part_status": [_vp],
        "mi_part_push_export": [_vp, _vp, _vp],
        "mi_part_push_connect": [_vp, _vp, _vp],
        "mi_part_spmv_push_dev": [_vp, _vp, _vp, _vp],
        "mi_part_push_info": [_vp, P(i), P(i), P(i)],
        "mi_part_sends_contiguous": [_vp, P(i)],
        "mi_part_combined_info": [_vp, P(i)],
        "mi_part_push_disable": [_vp],
        "mi_part_push_unfuse": [_vp],
        "mi_bcsr4_spmm": [_vp, i, _vp, ll, _vp, ll, i],
        "mi_bcsr4_spmm_info": [_vp, i, P(i), P(i), P(i), P(d)],
        "mi_bcsr4_spmm_dev": [_vp, i, _vp, ll, _vp, ll, i, _vp],
        "mi_spmm_dev": [_vp, i, _vp, ll, _vp, ll, _vp],
        "mi_krylov_basis_dev": [_vp, i, _vp, _vp, ll, i, _vp, _vp],
        "mi_krylov_basis_cgs_dev": [_vp, i, _vp, _vp, ll, i, _vp, _vp],
        "mi_csr_reorder_info": [_vp, P(i), P(i), P(d), P(d), P(d), P(d)],
        "mi_reorder_probe": [i, _vp, _vp, P(i), _vp, P(d), P(d)],
        "mi_csr_perm": [_vp, P(i), _vp],
        "mi_vec_to_internal_dev": [_vp, _vp, _vp, _vp],
        "mi_vec_from_internal_dev": [_vp, _vp, _vp, _vp],
        "mi_spmv_internal_dev": [_vp, _vp, _vp, _vp],
        "mi_spmk_internal_dev": [_vp, i, _vp, _vp, _vp],
        "mi_csr_dims": [_vp, P(i), P(i), P(ll)],
        "mi_csr_set_kernel": [_vp, i],
        "mi_csr_get_kernel": [_vp, P(i)],
        "mi_csr_ring_info": [_vp, P(i), P(i), P(i), P(d)],
        "mi_csr_ring_shape_info": [_vp, P(i), P(i), P(i), P(d), P(d)],
        "mi_csr_tune_info": [_vp, P(d), P(d)],
        "mi_csr_tune_detail": [_vp, P(d), P(_c.c_int), P(_c.c_int)],
        "mi_csr_set_nontemporal": [_vp, i, i],
        "mi_csr_block4_structure": [i, _vp, _vp, P(i), P(_c.c_longlong)],
        "mi_ring_plan_probe": [i, _vp, _vp, i, P(i), P(i), P(i), P(d), P(i)],
        "mi_ring_plan_lean": [i, _vp, _vp, i, P(i)],
        "mi_ring_plan_census": [i, _vp, _vp, i, _vp, i],
        "mi_mring_plan_census": [i, _vp, _vp, _vp, i],
        "mi_rowblock_census": [i, _vp, _vp, i, _vp, i],
        "mi_csr_stream_info": [_vp, P(i), P(i)],
        "mi_csr_tile_info": [_vp, P(i), P(i), P(d), P(d), P(i)],
        "mi_bcsr4_tile_info": [_vp, P(i), P(i), P(d), P(d)],
        "mi_bcsr4_tile_probe": [i, _vp, _vp, P(i), P(i), P(i), P(i)],
        "mi_bcsr4_sell_info": [_vp, P(i), P(i), P(ll), P(d), P(d)],
        "mi_bcsr4_sell_plan_probe": [i, _vp, _vp, i, P(i), P(ll), P(i), _vp, _vp, _vp],
        "mi_bcsr4_spmm_plan_probe": [i, _vp, _vp, i, i, P(i), P(i), P(i), P(d), _vp, ll, _vp, ll, _vp, ll, _vp, ll],
        "mi_csr_mring_info": [_vp, P(i), P(i), P(i), P(d), P(d), P(i)],
        "mi_csr_sstream_info": [_vp, P(i), P(i), P(ll), P(d), P(d), P(i)],
        "mi_sstream_plan_probe": [i, i, _vp, _vp, P(i), P(i), P(ll), P(d)],
        "mi_sstream_plan_probe_ex": [i, i, _vp, _vp, i, i, i, P(i), P(i), P(ll), P(d), P(i), P(i)],
        "mi_sstream_mw_plan_probe": [i, i, _vp, _vp, i, P(i), P(i), P(ll), P(d)],
        "mi_csr_placement_info": [_vp, P(i), P(i), P(d), i],
        "mi_vec_alloc_placed": [_vp, i, i, P(_vp), P(d), i, P(i)],
        "mi_vec_free_placed": [_vp],
        "mi_mring_plan_deal_probe": [i, _vp, _vp, P(i), _vp, i],
        "mi_mring_plan_probe": [i, _vp, _vp, P(i), P(i), P(i), P(d), P(ll)],
        "mi_tile_plan_probe": [i, _vp, _vp, i, P(i), P(ll), P(i), P(ll)],
        "mi_stream_read_probe": [ll, i, P(d)],
        "mi_spmv": [_vp, _vp, _vp],
        "mi_spmv_dev": [_vp, _vp, _vp, _vp],
        "mi_spmk": [_vp, i, _vp, _vp],
        "mi_spmk_dev": [_vp, i, _vp, _vp, _vp],
        "mi_csr_spmk_info": [_vp, i, P(i), P(i), P(d), P(d)],
        "mi_spmk_plan_probe": [i, _vp, _vp, P(i), P(i), P(i)],
        "mi_spmk_plan_dump": [i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, i, i, i],
        "mi_dot": [i, _vp, _vp, P(d)],
        "mi_dot_dev": [i, _vp, _vp, _vp, _vp],
        "mi_axpy": [i, d, _vp, _vp],
        "mi_axpy_dev": [i, d, _vp, _vp, _vp],
        "mi_orthogonalize": [i, _vp, _vp, _vp, d, P(d)],
        "mi_orthogonalize_dev": [i, _vp, _vp, _vp, d, _vp, _vp],
        "mi_spmv_dot_dev": [_vp, _vp, _vp, _vp, _vp, _vp],
        "mi_csr_dot_epilogue_info": [_vp, P(i)],
        "mi_csr_dot_epilogue_layout": [_vp, P(i), P(i), P(i), _vp, _vp, _vp, i, i],
        "mi_spmv_orthogonalize_dev": [_vp, _vp, _vp, _vp, _vp, d, _vp, _vp],
        "mi_norm2": [i, _vp, P(d)],
        "mi_norm2_dev": [i, _vp, _vp, _vp],
        "mi_rel_error": [i, _vp, _vp, P(d)],
        "mi_rel_error_dev": [i, _vp, _vp, _vp, _vp],
        "mi_gather_dev": [i, _vp, _vp, _vp, _vp],
        "mi_bcsr4_create": [i, i, _vp, _vp, _vp, P(_vp)],
        "mi_bcsr4_destroy": [_vp],
        "mi_bcsr4_create_layout": [i, i, _vp, _vp, _vp, i, P(_vp)],
        "mi_bcsr4_update_values_layout": [_vp, _vp, i],
        "mi_bcsr4_update_values_layout_dev": [_vp, _vp, i, _vp],
        "mi_bcsr4_spmv": [_vp, _vp, _vp],
        "mi_bcsr4_spmv_dev": [_vp, _vp, _vp, _vp],
        "mi_bcsr4_spmk": [_vp, i, _vp, _vp],
        "mi_bcsr4_spmk_dev": [_vp, i, _vp, _vp, _vp],
        "mi_bilu4_create": [i, _vp, _vp, _vp, i, i, P(_vp)],
        "mi_bilu4_create_host": [i, _vp, _vp, _vp, i, i, P(_vp)],
        "mi_bilu4_destroy": [_vp],
        "mi_bilu4_refactor": [_vp, _vp, i],
        "mi_bilu4_solve_dev": [_vp, _vp, _vp, _vp],
        "mi_bilu4_solve": [_vp, _vp, _vp],
        "mi_bilu4_info": [_vp, P(i), P(ll), P(i), P(i), P(i), P(i), P(d), P(d), P(ll)],
        "mi_bilu4_factor_host": [_vp, _vp, _vp, _vp, _vp, ll],
        "mi_bilu4_plan_probe": [i, _vp, _vp, i, P(ll), P(i), P(i), P(i), P(i), _vp, _vp, i],
        "mi_bilu4dev_plan_probe": [i, _vp, _vp, i, P(ll), P(i), P(ll)],
        "mi_bilu4dev_prepare": [_vp],
        "mi_bilu4dev_refactor": [_vp, _vp, i, _vp],
        "mi_bilu4dev_status": [_vp, P(i)],
        "mi_bilu4dev_fetch": [_vp],
        "mi_bilu4dev_info": [_vp, P(i), P(i), P(ll)],
        "mi_bilu4one_plan_probe": [i, _vp, _vp, i, i, P(i), _vp, _vp, P(ll), _vp, _vp, _vp, _vp],
        "mi_bilu4one_prepare": [_vp],
        "mi_bilu4_set_solve_form": [_vp, i],
        "mi_bilu4one_status": [_vp],
        "mi_bilu4one_info": [_vp, P(i), P(i), P(i), _vp, _vp, P(ll)],
        "mi_bilu4sw_prepare": [_vp],
        "mi_bilu4sw_solve_dev": [_vp, _vp, _vp, i, i, _vp],
        "mi_bilu4sw_solve": [_vp, _vp, _vp, i, i],
        "mi_bilu4sw_info": [_vp, P(i), P(i), P(i), P(i), P(ll)],
        "mi_bilu4sp_prepare": [_vp],
        "mi_bilu4sp_solve_dev": [_vp, _vp, _vp, i, i, _vp],
        "mi_bilu4sp_solve": [_vp, _vp, _vp, i, i],
        "mi_bilu4sp_status": [_vp, P(i), P(ll)],
        "mi_bilu4sp_fetch": [_vp, _vp, ll],
        "mi_bilu4sp_info": [_vp, P(i), P(i), P(i), P(ll)],
        "mi_bilu4spx_solve_dev": [_vp, _vp, _vp, _vp],
        "mi_bilu4spx_solve": [_vp, _vp, _vp],
        "mi_bilu4spx_info": [_vp, P(i), P(i)],
        "mi_bilu4_create_ordered": [i, _vp, _vp, _vp, i, i, i, P(_vp)],
        "mi_bilu4_create_host_ordered": [i, _vp, _vp, _vp, i, i, i, P(_vp)],
        "mi_bilu4_order_info": [_vp, P(i), P(i), P(i), _vp],
        "mi_bilu4_order_probe": [i, _vp, _vp, i, _vp, P(i), _vp, i],
        "mi_gmres_create": [i, i, P(_vp)],
        "mi_gmres_set_operator_csr": [_vp, _vp],
        "mi_gmres_set_operator_bcsr4": [_vp, _vp],
        "mi_gmres_set_precond": [_vp, _vp, i, i, i],
        "mi_gmres_set_precond_ex": [_vp, _vp, i, i, i],
        "mi_gmres_solve_dev": [_vp, _vp, _vp, d, i, i, P(i), P(i), _vp, _vp],
        "mi_gmres_solve": [_vp, _vp, _vp, d, i, i, P(i), P(i), _vp],
        "mi_gmres_fetch_cycle": [_vp, P(i), _vp, _vp, P(d)],
        "mi_gmres_info": [_vp, P(i), P(ll), P(i), P(i), P(i)],
        "mi_gmres_destroy": [_vp],
        "mi_gmres_create_ex": [i, i, i, P(_vp)],
        "mi_gmres_basis_info": [_vp, P(i), P(ll), P(i)],
        "mi_round_f32_dev": [i, _vp, _vp, _vp, _vp, _vp],
        "mi_mdot_f32_dev": [i, i, _vp, _vp, _vp, _vp],
        "mi_maxpy_f32_dev": [i, i, _vp, i, _vp, _vp, _vp, _vp],
        "mi_cgs_f32_dev": [i, i, _vp, _vp, i, _vp, _vp, _vp],
        "mi_maxpy_upto_dev": [i, i, _vp, _vp, i, _vp, _vp, _vp],
        "mi_maxpy_upto_f32_dev": [i, i, _vp, _vp, i, _vp, _vp, _vp],
        "mi_gmres_prepare_stream": [_vp, _vp],
        "mi_gmres_cycle_dev": [_vp, _vp, _vp, i, d, i, _vp],
        "mi_gmres_state": [_vp, _vp, P(i), P(i), P(i), P(i), P(d), P(d), _vp],
        "mi_gmres_plan_create": [_vp, _vp, _vp, d, i, i, P(_vp)],
        "mi_gmres_plan_solve": [_vp, P(i), P(i), _vp, _vp],
        "mi_gmres_plan_info": [_vp, P(i), P(i), P(i), P(i), P(i)],
        "mi_gmres_plan_destroy": [_vp],
        "mi_dilu4_create": [i, _vp, _vp, _vp, i, i, P(_vp)],
        "mi_dilu4_create_host": [i, _vp, _vp, _vp, i, i, P(_vp)],
        "mi_dilu4_destroy": [_vp],
        "mi_dilu4_refactor": [_vp, _vp, i],
        "mi_dilu4_fetch": [_vp, _vp, _vp],
        "mi_dilu4_info": [_vp, P(i), P(ll), P(i), P(i), P(i), P(i), P(i), P(d), P(ll), _vp],
        "mi_dilu4_to_hat_dev": [_vp, _vp, _vp, _vp],
        "mi_dilu4_from_hat_dev": [_vp, _vp, _vp, _vp],
        "mi_dilu4_apply_hat_dev": [_vp, _vp, _vp, _vp],
        "mi_gmres_set_operator_dilu4": [_vp, _vp],
        "mi_dilu4dev_plan_probe": [i, _vp, _vp, i, P(ll), P(i), P(ll)],
        "mi_dilu4dev_prepare": [_vp],
        "mi_dilu4dev_refactor": [_vp, _vp, i, _vp],
        "mi_dilu4dev_status": [_vp, P(i)],
        "mi_dilu4dev_fetch": [_vp],
        "mi_dilu4dev_info": [_vp, P(i), P(i), P(ll)],
        "mi_part_create": [i, i, _vp, _vp, _vp, _vp, P(_vp)],
        "mi_part_destroy": [_vp],
        "mi_part_sizes": [_vp, P(i), P(i), P(i), P(i)],
        "mi_part_recv_counts": [_vp, _vp],
        "mi_part_recv_ids": [_vp, i, _vp],
        "mi_part_set_send_ids": [_vp, i, i, _vp],
        "mi_part_send_counts": [_vp, _vp],
        "mi_part_local_csr": [_vp, i, P(i), P(_vp), P(_vp), P(_vp), P(_vp)],
        "mi_part_send_index": [_vp, P(i), P(_vp)],
        "mi_part_finalize": [_vp],
        "mi_part_set_kernel": [_vp, i],
        "mi_part_update_values": [_vp, _vp],
        "mi_part_pack_dev": [_vp, _vp, _vp, _vp],
        "mi_part_spmv_interior_dev": [_vp, _vp, _vp, _vp],
        "mi_part_spmv_boundary_dev": [_vp, _vp, _vp, _vp],
        "mi_comm_available": [],
        "mi_comm_unique_id": [_vp],
        "mi_part_comm_init": [_vp, _vp],
        "mi_part_comm_info": [_vp, P(i), P(i)],
        "mi_part_spmv_dev": [_vp, _vp, _vp, _vp],
        "mi_comm_selftest": [i, P(d)],
        "mi_part_send_union": [_vp, P(i), P(_vp)],
        "mi_part_allgather_setup": [_vp, _vp, _vp],
        "mi_part_set_allgather": [_vp, i],
        "mi_part_allgather_info": [_vp, P(i), P(i), P(i)],
        "mi_dist_create": [i, i, _vp, _vp, _vp, P(_vp)],
        "mi_dist_destroy": [_vp],
        "mi_dist_info": [_vp, P(i), P(i), P(i), P(i), P(ll), P(ll)],
        "mi_dist_rank_info": [_vp, i, P(i), P(ll), P(i), P(i), P(ll), P(_vp)],
        "mi_dist_update_values": [_vp, _vp],
        "mi_dist_spmv": [_vp, _vp, _vp],
        "mi_dist_spmk": [_vp, i, _vp, _vp],
        "mi_dist_dot": [_vp, _vp, _vp, P(d)],
        "mi_dist_orthogonalize": [_vp, _vp, _vp, _vp, d, P(d)],
        "mi_dist_vec_create": [_vp, P(_vp)],
        "mi_dist_vec_destroy": [_vp],
        "mi_dist_vec_set": [_vp, _vp],
        "mi_dist_vec_get": [_vp, _vp],
        "mi_dist_vec_ptr": [_vp, i, P(_vp)],
        "mi_dist_spmv_dev": [_vp, _vp, _vp],
        "mi_dist_spmk_dev": [_vp, i, _vp, _vp],
        "mi_dist_synchronize": [_vp],
        "mi_dist_dot_dev": [_vp, _vp, _vp, P(d)],
        "mi_dist_orthogonalize_dev": [_vp, _vp, _vp, _vp, d, P(d)],
    }
    for name, argt in sigs.items():
        fn = getattr(L, name)
        fn.argtypes = argt
        fn.restype = _c.c_int
    for name in ("mi_dist_exchange_name", "mi_dist_exchange_note"):
        getattr(L, name).argtypes = [_vp]
        getattr(L, name).restype = _c.c_char_p
    L.mi_part_kernel_name.argtypes = [_vp, i]
    L.mi_part_kernel_name.restype = _c.c_char_p
    # diagnostics of include/mi355_devtools.h: present only in libmi355spmv_dev.so (`make devtools`; tools/ load it through
    # MI355_SPMV_LIBRARY), never in the product library
    for name, argt in {"mi_debug_xcc_map": [i, _vp], "mi_debug_touch_pages": [_vp, i, _vp, ll, _vp, ll],
                       "mi_part_push_debug_preset": [_vp, _c.c_uint], "mi_debug_part_push_trace": [_vp, _vp, _vp, i, _vp, P(i), _vp],
                       "mi_debug_part_ext_mode": [_vp, i], "mi_debug_part_ext_trace": [_vp, _vp, _vp, i, _vp, P(i), _vp],
                       "mi_debug_spmk_set_epoch": [_vp, _c.c_uint]}.items():
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.argtypes = argt
            fn.restype = _c.c_int
    _LIB = L
    return L


def check(status):
    if status != MI_OK:
        raise MiError(status, lib().mi_last_error().decode(errors="replace"))


# ----------------------------------------------------------------- plumbing

def _is_torch(t):
    return type(t).__module__.startswith("torch")


def _stream_ptr():
    import torch

    return _vp(torch.cuda.current_stream().cuda_stream)


def _dev_ptr(t, n=None, what="vector", dtype=None):
    import torch

    dtype = dtype or torch.float64
    if not (t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise TypeError(f"{what}: expected a contiguous {str(dtype)[6:]} CUDA tensor, got {t.dtype} on {t.device}")
    if n is not None and t.numel() < n:
        raise ValueError(f"{what}: needs {n} entries, has {t.numel()}")
    return _vp(t.data_ptr())


def _host_f64(a, n=None, what="vector", writable=False):
    if not isinstance(a, np.ndarray) or a.dtype != np.float64 or not a.flags.c_contiguous:
        if writable:
            raise TypeError(f"{what}: output must be a C-contiguous float64 numpy array")
        a = np.ascontiguousarray(a, dtype=np.float64)
    if n is not None and a.size < n:
        raise ValueError(f"{what}: needs {n} entries, has {a.size}")
    return a


# ------------------------------------------------------------------ matrices

class csrmatrix:
    """struct csrmatrix of mpk/SpMV.h:18-24 — n, nnz, ptrow, indcol, coef — plus the
    device handle (lazily created; the matrix is immutable once used)."""

    def __init__(self, n, ptrow, indcol, coef, ncols=None, rowmap=None):
        self.n = int(n)
        self.ptrow = np.ascontiguousarray(ptrow, dtype=np.int32)
        self.indcol = np.ascontiguousarray(indcol, dtype=np.int32)
        self.coef = np.ascontiguousarray(coef, dtype=np.float64)
        if len(self.ptrow) != self.n + 1:
            raise ValueError("ptrow must have n+1 entries")
        self.nnz = int(self.ptrow[-1]) if self.n > 0 else 0
        self.ncols = self.n if ncols is None else int(ncols)
        self.rowmap = None if rowmap is None else np.ascontiguousarray(rowmap, dtype=np.int32)
        self._h = None
        self._kernel = KERNEL_AUTO

    @property
    def handle(self):
        if self._h is None:
            h = _vp()
            if self.rowmap is None:
                check(lib().mi_csr_create(self.n, self.ncols, self.ptrow.ctypes.data, self.indcol.ctypes.data,
                                          self.coef.ctypes.data, _c.byref(h)))
            else:
                check(lib().mi_csr_create_mapped(self.n, self.ncols, self.ptrow.ctypes.data, self.indcol.ctypes.data,
                                                 self.coef.ctypes.data, self.rowmap.ctypes.data, _c.byref(h)))
            self._h = h
            if self._kernel != KERNEL_AUTO:
                check(lib().mi_csr_set_kernel(h, self._kernel))
        return self._h

    def set_kernel(self, kernel):
        kid = KERNELS[kernel] if isinstance(kernel, str) else int(kernel)
        self._kernel = kid
        if self._h is not None:
            check(lib().mi_csr_set_kernel(self._h, kid))
        return self

    def kernel_name(self):
        return lib().mi_csr_kernel_name(self.handle).decode()

    def ring_info(self):
        """(config id, runs, runs not served by the ring, fraction of nonzeros the ring serves)."""
        cfg, runs, bad = _c.c_int(), _c.c_int(), _c.c_int()
        frac = _c.c_double()
        check(lib().mi_csr_ring_info(self.handle, _c.byref(cfg), _c.byref(runs), _c.byref(bad), _c.byref(frac)))
        return cfg.value, runs.value, bad.value, frac.value

    def ring_shape_info(self):
        """dict(blocks, lean, depth, us_aligned, us_unaligned) — mi_csr_ring_shape_info."""
        b, l, dd = _c.c_int(), _c.c_int(), _c.c_int()
        ua, uu = _c.c_double(), _c.c_double()
        check(lib().mi_csr_ring_shape_info(self.handle, _c.byref(b), _c.byref(l), _c.byref(dd), _c.byref(ua), _c.byref(uu)))
        return dict(blocks=b.value, lean=bool(l.value), depth=dd.value, us_aligned=ua.value, us_unaligned=uu.value)

    def tune_info(self):
        """(us per launch measured for ring, for stream) at create time; zeros if not measured."""
        a, b = _c.c_double(), _c.c_double()
        check(lib().mi_csr_tune_info(self.handle, _c.byref(a), _c.byref(b)))
        return a.value, b.value

    def tune_detail(self):
        """(us per launch measured at create time for ring / stream, each with temporal and non-temporal
        matrix loads; whether the kernel that AUTO resolves to uses non-temporal loads)."""
        us = (_c.c_double * 5)()
        rnt, snt = _c.c_int(), _c.c_int()
        check(lib().mi_csr_tune_detail(self.handle, us, _c.byref(rnt), _c.byref(snt)))
        nt = rnt.value if "ring" in self.kernel_name() else snt.value
        out = dict(ring=us[0], ring_nt=us[1], stream=us[2], stream_nt=us[3], bcsr4=us[4])
        m = self.mring_info()
        if m["built"]:
            out.update(mring=m["us"], mring_nt=m["us_nt"])
            if "mring" in self.kernel_name():
                nt = m["nt"]
        t = self.tile_info()
        if t["built"]:
            out.update(tile=t["us"], tile_nt=t["us_nt"])
            if "tile" in self.kernel_name():
                nt = t["nt"]
        return out, bool(nt)

    def placement_info(self):
        """dict(values=[us as first allocated, us after each draw ...], column_stream=[...]) — mi_csr_placement_info (create-time placement draws)."""
        nv, nt = _c.c_int(), _c.c_int()
        us = (_c.c_double * 32)()
        check(lib().mi_csr_placement_info(self.handle, _c.byref(nv), _c.byref(nt), us, 32))
        return dict(values=[round(us[k], 2) for k in range(nv.value)], column_stream=[round(us[k], 2) for k in range(nv.value, nt.value)])

    def alloc_vectors(self, nvec=2, draws=8):
        """nvec device vectors (torch float64 tensors of length n, zero-filled) placed for products with this matrix —
        mi_vec_alloc_placed: the library allocates `draws` candidate x / y pairs, times y = A x on each and keeps the fastest
        (where a vector lies in device memory moves a product by up to 12 % on some boxes, profiles/NOTES.md §4.12).
        Returns (tensors, us_per_candidate_pair).  The memory belongs to the returned tensors' `_placed` owner: it is released
        when the last of them is garbage-collected."""
        import torch
        ptrs = (_vp * nvec)()
        us = (_c.c_double * 64)()
        nus = _c.c_int()
        check(lib().mi_vec_alloc_placed(self.handle, nvec, draws, ptrs, us, 64, _c.byref(nus)))
        out = []
        for k in range(nvec):
            buf = _PlacedBuffer(int(ptrs[k]), max(self.n, self.ncols))
            t = torch.as_tensor(buf, device="cuda")[: self.n]
            t._placed = buf  # keeps the allocation alive as long as the tensor object lives
            out.append(t)
        return out, [round(us[k], 2) for k in range(nus.value)]

    def mring_info(self):
        """dict(built, runs, runs_not_served, nnz_fraction, us, us_nt, nt) — mi_csr_mring_info (multi-window ring plan)."""
        b, r, bad, nt = _c.c_int(), _c.c_int(), _c.c_int(), _c.c_int()
        f = _c.c_double()
        us = (_c.c_double * 2)()
        check(lib().mi_csr_mring_info(self.handle, _c.byref(b), _c.byref(r), _c.byref(bad), _c.byref(f), us, _c.byref(nt)))
        return dict(built=bool(b.value), runs=r.value, runs_not_served=bad.value, nnz_fraction=f.value, us=us[0], us_nt=us[1],
                    nt=bool(nt.value))

    def sstream_info(self):
        """dict(built, rounds, steps, padding, us_d8_nt, us_d8_temporal, us_d12_nt, us_d12_temporal, form) — mi_csr_sstream_info (sliced-stream kernel)."""
        b, r, fm = _c.c_int(), _c.c_int(), _c.c_int()
        st = _c.c_longlong()
        pad = _c.c_double()
        us = (_c.c_double * 4)()
        check(lib().mi_csr_sstream_info(self.handle, _c.byref(b), _c.byref(r), _c.byref(st), _c.byref(pad), us, _c.byref(fm)))
        return dict(built=bool(b.value), rounds=r.value, steps=st.value, padding=pad.value, us_d8_nt=us[0], us_d8_temporal=us[1], us_d12_nt=us[2],
                    us_d12_temporal=us[3], form=fm.value)

    def tile_info(self):
        """dict(built, nblk, unique_per_nnz, us, us_nt, nt) — mi_csr_tile_info (the tile kernel's plan on this handle)."""
        b, nb, nt = _c.c_int(), _c.c_int(), _c.c_int()
        u = _c.c_double()
        us = (_c.c_double * 2)()
        check(lib().mi_csr_tile_info(self.handle, _c.byref(b), _c.byref(nb), _c.byref(u), us, _c.byref(nt)))
        return dict(built=bool(b.value), nblk=nb.value, unique_per_nnz=u.value, us=us[0], us_nt=us[1], nt=bool(nt.value))

    def stream_info(self):
        """dict(nblk, row_align) — mi_csr_stream_info (the handle's table for the stream kernel, built if no product needed it yet)."""
        nb, al = _c.c_int(), _c.c_int()
        check(lib().mi_csr_stream_info(self.handle, _c.byref(nb), _c.byref(al)))
        return dict(nblk=nb.value, row_align=al.value)

    def reorder_info(self):
        """dict(reordered, block, spread_before, spread_after, us_natural, us_reordered) — mi_csr_reorder_info."""
        r, b = _c.c_int(), _c.c_int()
        v = [_c.c_double() for _ in range(4)]
        check(lib().mi_csr_reorder_info(self.handle, _c.byref(r), _c.byref(b), *[_c.byref(t) for t in v]))
        return dict(reordered=bool(r.value), block=b.value, spread_before=v[0].value, spread_after=v[1].value,
                    us_natural=v[2].value, us_reordered=v[3].value)

    def spmk_info(self, k):
        """dict(eligible, one_launch, us_k_launches, us_one_launch): how this handle runs the k-step (mi_csr_spmk_info)."""
        e, o = _c.c_int(), _c.c_int()
        a, b = _c.c_double(), _c.c_double()
        check(lib().mi_csr_spmk_info(self.handle, int(k), _c.byref(e), _c.byref(o), _c.byref(a), _c.byref(b)))
        return dict(eligible=bool(e.value), one_launch=bool(o.value), us_k_launches=a.value, us_one_launch=b.value)

    def dot_in_epilogue(self):
        """True if SpMV_CSR_dot / SpMV_CSR_orthogonalize on this handle carry the dot inside the product's launch."""
        r = _c.c_int()
        check(lib().mi_csr_dot_epilogue_info(self.handle, _c.byref(r)))
        return bool(r.value)

    def dot_epilogue_layout(self):
        """What the dot epilogue walks (mi_csr_dot_epilogue_layout): dict(threads, run_first_block [wgs + 1], block_row0 [nblk],
        block_rows [nblk]).  Raises MiError on a handle whose launch does not carry the dot."""
        t, w, nb = _c.c_int(), _c.c_int(), _c.c_int()
        check(lib().mi_csr_dot_epilogue_layout(self.handle, _c.byref(t), _c.byref(w), _c.byref(nb), None, None, None, 0, 0))
        first = np.zeros(w.value + 1, np.int32)
        row0 = np.zeros(max(nb.value, 1), np.int32)
        rows = np.zeros(max(nb.value, 1), np.int32)
        check(lib().mi_csr_dot_epilogue_layout(self.handle, _c.byref(t), _c.byref(w), _c.byref(nb), first.ctypes.data,
                                               row0.ctypes.data, rows.ctypes.data, first.size, row0.size))
        return dict(threads=t.value, run_first_block=first, block_row0=row0[: nb.value], block_rows=rows[: nb.value])

    # -- the library's numbering (mi_csr_perm ...): permute once per solve, not once per product --------------------
    def perm(self):
        """(reordered, perm) with perm[old] = new — identity when the handle was not relabelled."""
        r = _c.c_int()
        p = np.empty(self.n, np.int32)
        check(lib().mi_csr_perm(self.handle, _c.byref(r), p.ctypes.data))
        return bool(r.value), p

    def to_internal(self, x, out=None):
        import torch
        out = torch.empty_like(x) if out is None else out
        check(lib().mi_vec_to_internal_dev(self.handle, _dev_ptr(x, self.n, "x"), _dev_ptr(out, self.n, "x_int"), _stream_ptr()))
        return out

    def from_internal(self, x_int, out=None):
        import torch
        out = torch.empty_like(x_int) if out is None else out
        check(lib().mi_vec_from_internal_dev(self.handle, _dev_ptr(x_int, self.n, "x_int"), _dev_ptr(out, self.n, "x"), _stream_ptr()))
        return out

    def update_values(self, coef):
        """New coefficients for the same pattern (mi_csr_update_values): numpy array (host) or CUDA tensor."""
        if _is_torch(coef):
            check(lib().mi_csr_update_values_dev(self.handle, _dev_ptr(coef, self.nnz, "coef"), _stream_ptr()))
        else:
            self.coef = _host_f64(coef, self.nnz, "coef")
            check(lib().mi_csr_update_values(self.handle, self.coef.ctypes.data))
        return self

    def drop_host_arrays(self):
        """Free the host copies of indcol/coef once the device handle exists (large benches)."""
        _ = self.handle
        self.indcol = self.indcol[:0]
        self.coef = self.coef[:0]

    def close(self):
        if self._h is not None:
            lib().mi_csr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class bcsr4x4_matrix:
    """struct bcsr4x4_matrix of mpk/SpMV.h:26-33 (row-major 4x4 blocks)."""

    def __init__(self, nrows, ptrow, indcol, coef, nbcols=None, layout="row"):
        """layout: "row" — blocks row-major as mpk/ stores them; "col" — column-major as PETSc's MATSEQBAIJ stores them
        (src/kernels/baij4_mad.c:73-76), transposed by the library on upload."""
        self.layout = {"row": 0, "col": 1}[layout]
        self.nrows = int(nrows)
        self.ptrow = np.ascontiguousarray(ptrow, dtype=np.int32)
        self.indcol = np.ascontiguousarray(indcol, dtype=np.int32)
        self.coef = np.ascontiguousarray(coef, dtype=np.float64)
        self.nblocks = len(self.indcol)
        self.nbcols = (int(self.indcol.max()) + 1 if self.nblocks else 0) if nbcols is None else int(nbcols)
        self.nbcols = max(self.nbcols, self.nrows)
        self._h = None

    @property
    def handle(self):
        if self._h is None:
            h = _vp()
            check(lib().mi_bcsr4_create_layout(self.nrows, self.nbcols, self.ptrow.ctypes.data, self.indcol.ctypes.data,
                                               self.coef.ctypes.data, self.layout, _c.byref(h)))
            self._h = h
        return self._h

    def update_values(self, coef):
        """New block values (same pattern, same layout as at construction): numpy array or CUDA tensor."""
        if _is_torch(coef):
            check(lib().mi_bcsr4_update_values_layout_dev(self.handle, _dev_ptr(coef, 16 * self.nblocks, "coef"), self.layout, _stream_ptr()))
        else:
            self.coef = _host_f64(coef, 16 * self.nblocks, "coef")
            check(lib().mi_bcsr4_update_values_layout(self.handle, self.coef.ctypes.data, self.layout))
        return self

    def close(self):
        if self._h is not None:
            lib().mi_bcsr4_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


GMRES_PC_EXACT, GMRES_PC_SWEEPS, GMRES_PC_SWEEPS_F32, GMRES_PC_EXACT_F32 = 0, 1, 2, 3  # MI_GMRES_PC_*

# the ways a factor is applied, (sweeps, f32) -> the entry point for device vectors, the one for host vectors, the kind GMRES knows it by
_BILU_APPLY = {
    (False, False): ("mi_bilu4_solve_dev", "mi_bilu4_solve", GMRES_PC_EXACT),
    (True, False): ("mi_bilu4sw_solve_dev", "mi_bilu4sw_solve", GMRES_PC_SWEEPS),
    (True, True): ("mi_bilu4sp_solve_dev", "mi_bilu4sp_solve", GMRES_PC_SWEEPS_F32),
    (False, True): ("mi_bilu4spx_solve_dev", "mi_bilu4spx_solve", GMRES_PC_EXACT_F32),
}


def _bilu_solve(F, way, counts, x, b):
    """x = the factor of F (a bilu4) applied to b in that way (a row of _BILU_APPLY); counts: (fwd, bwd) of a sweep solve, else ().
    CUDA tensors: asynchronous on torch's current stream, x may be b; numpy arrays: copied in and out."""
    n = 4 * F.nbrows
    dev, host, _ = way
    if _is_torch(b):
        check(getattr(lib(), dev)(F.handle, _dev_ptr(b, n, "b"), _dev_ptr(x, n, "x"), *counts, _stream_ptr()))
    else:
        xx = _host_f64(x, n, "x", writable=True)
        check(getattr(lib(), host)(F.handle, _host_f64(b, n, "b").ctypes.data, xx.ctypes.data, *counts))
    return x


def _block_pattern(A, ptrow, indcol, coef, layout):
    """What bilu4 and dilu4 are made from, checked: (nbrows, ptrow, indcol, coef, lay) of a bcsr4x4_matrix A (its host arrays and
    block layout), or of the arrays themselves with A the number of block rows."""
    if isinstance(A, bcsr4x4_matrix):
        nbrows, ptrow, indcol, coef, lay = A.nrows, A.ptrow, A.indcol, A.coef, A.layout
    else:
        nbrows, lay = int(A), {"row": 0, "col": 1}[layout]
    ptrow = np.ascontiguousarray(ptrow, dtype=np.int32)
    indcol = np.ascontiguousarray(indcol, dtype=np.int32)
    coef = _host_f64(coef, None, "coef")
    if len(ptrow) != int(nbrows) + 1:
        raise ValueError("ptrow must have nbrows+1 entries")
    if coef.size < 16 * len(indcol):
        raise ValueError("coef: 16 values per block")
    return int(nbrows), ptrow, indcol, coef, lay


class _OwnsHandle:
    """The C handle self._h of a bilu4 or a dilu4: refused once closed, destroyed (by the class's _destroy symbol) exactly once."""
    _h, _destroy = None, None

    @property
    def handle(self):
        if self._h is None:
            raise ValueError(f"{type(self).__name__}: closed")
        return self._h

    def close(self):
        if self._h is not None:
            getattr(lib(), self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class bilu4(_OwnsHandle):
    """mi_bilu4_t: the incomplete LU factors of a square 4x4-block matrix — PCILU on the BAIJ-4 Jacobian,
    src/solve_newton.c:1156-1164 — factored on the host at construction, solved on the GPU level by level.
    bilu4(A, fill=0) takes a bcsr4x4_matrix's host arrays (and its block layout); bilu4(nbrows, ptrow, indcol, coef, fill=0,
    layout="row") the arrays themselves.  host_only=True: no device copy (pattern, schedule and factor values only).
    order="colour" (mi_bilu4_create_ordered): the factor of the matrix under a multicolour renumbering of its block rows — a
    different, usually weaker preconditioner whose exact solve has about as many levels as colours; opt-in, never chosen for
    you.  Every method keeps the caller's numbering except factor_host() and fetch_f32(), which return the permuted matrix's
    factor; one solve at a time per ordered handle."""

    _destroy = "mi_bilu4_destroy"

    def __init__(self, A, ptrow=None, indcol=None, coef=None, fill=0, layout="row", host_only=False, order="natural"):
        self.nbrows, ptrow, indcol, coef, lay = _block_pattern(A, ptrow, indcol, coef, layout)
        self.layout = lay
        self.fill = int(fill)
        self._nblocks_in = len(indcol)
        h = _vp()
        self.order = order
        if order == "natural":  # the entry points natural-order handles have always been made by
            make = lib().mi_bilu4_create_host if host_only else lib().mi_bilu4_create
            check(make(self.nbrows, ptrow.ctypes.data, indcol.ctypes.data, coef.ctypes.data, lay, self.fill, _c.byref(h)))
        else:
            make = lib().mi_bilu4_create_host_ordered if host_only else lib().mi_bilu4_create_ordered
            check(make(self.nbrows, ptrow.ctypes.data, indcol.ctypes.data, coef.ctypes.data, lay, self.fill, _bilu_order(order), _c.byref(h)))
        self._h = h

    def order_info(self):
        """dict(order, ncolours, wide_launches, perm) — mi_bilu4_order_info: perm[old block row] = new (the identity in natural
        order); wide_launches: launches of one exact solve in form 0 that take the wide-level kernel."""
        o, nc, wl = _c.c_int(), _c.c_int(), _c.c_int()
        perm = np.zeros(max(self.nbrows, 1), np.int32)
        check(lib().mi_bilu4_order_info(self.handle, _c.byref(o), _c.byref(nc), _c.byref(wl), perm.ctypes.data))
        return dict(order=BILU_ORDERS[o.value], ncolours=nc.value, wide_launches=wl.value, perm=perm[: self.nbrows])

    def solve(self, x, b):
        """x = U^-1 L^-1 b.  CUDA tensors: asynchronous on torch's current stream, x may be b; numpy arrays: copied in and out."""
        return _bilu_solve(self, _BILU_APPLY[False, False], (), x, b)

    def gmres_args(self):
        """(handle, MI_GMRES_PC_* kind, sweeps_fwd, sweeps_bwd): what gmres_solver sets this M with."""
        return self.handle, GMRES_PC_EXACT, 0, 0

    def refactor(self, coef):
        """New block values for the same pattern (same layout as at construction)."""
        coef = _host_f64(coef, 16 * self._nblocks_in, "coef")
        check(lib().mi_bilu4_refactor(self.handle, coef.ctypes.data, self.layout))
        return self

    def prepare_dev(self):
        """Build and upload the pattern-only tables of the device refactor (mi_bilu4dev_prepare; idempotent)."""
        check(lib().mi_bilu4dev_prepare(self.handle))
        return self

    def refactor_dev(self, coef):
        """New block values for the same pattern from a CUDA tensor (the order and layout of the arrays at construction), factored
        on the GPU into the device factor: asynchronous on torch's current stream (mi_bilu4dev_refactor).  A refused pivot shows
        in factor_status(); the host factor follows only after fetch_factor()."""
        check(lib().mi_bilu4dev_refactor(self.handle, _dev_ptr(coef, 16 * self._nblocks_in, "coef"), self.layout, _stream_ptr()))
        return self

    def factor_status(self):
        """Wait for the last refactor_dev; MiError (MI_ERR_ARG, naming the block row) when it refused a pivot."""
        bad = _c.c_int()
        check(lib().mi_bilu4dev_status(self.handle, _c.byref(bad)))
        return self

    def fetch_factor(self):
        """Copy the device factor back into the host factor, so that factor_host() returns what the device holds."""
        check(lib().mi_bilu4dev_fetch(self.handle))
        return self

    def info_dev(self):
        """dict(prepared, launches, plan_bytes) — mi_bilu4dev_info."""
        pr, la, by = _c.c_int(), _c.c_int(), _c.c_longlong()
        check(lib().mi_bilu4dev_info(self.handle, _c.byref(pr), _c.byref(la), _c.byref(by)))
        return dict(prepared=bool(pr.value), launches=la.value, plan_bytes=by.value)

    def set_form(self, form):
        """The form of this handle's solves (mi_bilu4_set_solve_form): 0 one launch per level, 1 both sweeps in one launch (MiError,
        status 5, when the pattern is not eligible), -1 measure both and keep the faster.  Returns the form now in use."""
        check(lib().mi_bilu4_set_solve_form(self.handle, int(form)))
        return self.info()["form"]

    def prepare_one(self):
        """Build and upload the tables of the one-launch form (mi_bilu4one_prepare; idempotent); MiError, status 5, when the pattern
        is not eligible."""
        check(lib().mi_bilu4one_prepare(self.handle))
        return self

    def one_status(self):
        """MiError (MI_ERR_HIP) once a hand-off wait of the one-launch form has given up (mi_bilu4one_status); no GPU work."""
        check(lib().mi_bilu4one_status(self.handle))
        return self

    def info_one(self):
        """dict(prepared, eligible, workgroups, nchunks, max_deps, plan_bytes) — mi_bilu4one_info; nchunks and max_deps are
        (forward, backward)."""
        pr, el, wg, by = _c.c_int(), _c.c_int(), _c.c_int(), _c.c_longlong()
        nch, md = (_c.c_int * 2)(), (_c.c_int * 2)()
        check(lib().mi_bilu4one_info(self.handle, _c.byref(pr), _c.byref(el), _c.byref(wg), nch, md, _c.byref(by)))
        return dict(prepared=bool(pr.value), eligible=bool(el.value), workgroups=wg.value, nchunks=(nch[0], nch[1]), max_deps=(md[0], md[1]),
                    plan_bytes=by.value)

    def sweeps(self, fwd, bwd=None, precision="f64"):
        """The same factor applied by `fwd` Jacobi sweeps of the forward triangle and `bwd` (default: fwd) of the backward one
        instead of the exact solve (mi_bilu4sw_*): a view with .solve(x, b), which is what GMRES takes as M.  Counts above
        levels - 1 are clamped: there the result is the exact solve's, bit for bit.  precision="f32": the sweeps stream the
        single-precision copy of the factor's values (mi_bilu4sp_*); vectors and arithmetic stay double."""
        return bilu4_apply(self, True, precision, fwd, fwd if bwd is None else bwd)

    def exact(self, precision="f64"):
        """The exact solve as a view with .solve(x, b), which GMRES takes as M like a sweeps() view.  precision="f64": the handle's
        own solve (the handle itself).  precision="f32": the level-by-level exact solve streaming the single-precision copy of the
        factor's values (mi_bilu4spx_*) — the exact solve of the rounded factor; vectors and arithmetic stay double.  The view
        shares this handle and owns nothing."""
        return bilu4_apply(self, False, precision) if _sweep_precision(precision) else self

    def exact_info_f32(self):
        """dict(launches_last, wide_launches_last) of the last single-precision exact solve — mi_bilu4spx_info."""
        la, wl = _c.c_int(), _c.c_int()
        check(lib().mi_bilu4spx_info(self.handle, _c.byref(la), _c.byref(wl)))
        return dict(launches_last=la.value, wide_launches_last=wl.value)

    def prepare_sweeps(self, precision="f64"):
        """Allocate the work vectors of the sweep solve (mi_bilu4sw_prepare; idempotent): needed before a graph capture.
        precision="f32": also the single-precision copy of the factor, converted now and kept current by every refactor
        (mi_bilu4sp_prepare)."""
        check((lib().mi_bilu4sp_prepare if _sweep_precision(precision) else lib().mi_bilu4sw_prepare)(self.handle))
        return self

    def sweep_status_f32(self):
        """Wait for the last conversion to single precision; MiError (MI_ERR_ARG, naming the block row; .bad_block_row and
        .overflowed on the exception) when finite values of the factor became Inf in the copy (mi_bilu4sp_status)."""
        bad, cnt = _c.c_int(), _c.c_longlong()
        status = lib().mi_bilu4sp_status(self.handle, _c.byref(bad), _c.byref(cnt))
        try:
            check(status)
        except MiError as e:
            e.bad_block_row, e.overflowed = bad.value, cnt.value
            raise
        return self

    def fetch_f32(self):
        """The single-precision copy as (nblocks, 4, 4) float32 in the host factor's block order (mi_bilu4sp_fetch)."""
        nblk = self.info()["nblocks"]
        val = np.zeros((max(nblk, 1), 4, 4), np.float32)
        check(lib().mi_bilu4sp_fetch(self.handle, val.ctypes.data, max(nblk, 1)))
        return val[:nblk]

    def sweep_info_f32(self):
        """dict(prepared, convert_launches, launches_last, copy_bytes) — mi_bilu4sp_info."""
        pr, cv, la, by = _c.c_int(), _c.c_int(), _c.c_int(), _c.c_longlong()
        check(lib().mi_bilu4sp_info(self.handle, _c.byref(pr), _c.byref(cv), _c.byref(la), _c.byref(by)))
        return dict(prepared=bool(pr.value), convert_launches=cv.value, launches_last=la.value, copy_bytes=by.value)

    def sweep_info(self):
        """dict(prepared, max_fwd, max_bwd, launches_last, work_bytes) — mi_bilu4sw_info."""
        pr, mf, mb, la, by = _c.c_int(), _c.c_int(), _c.c_int(), _c.c_int(), _c.c_longlong()
        check(lib().mi_bilu4sw_info(self.handle, _c.byref(pr), _c.byref(mf), _c.byref(mb), _c.byref(la), _c.byref(by)))
        return dict(prepared=bool(pr.value), max_fwd=mf.value, max_bwd=mb.value, launches_last=la.value, work_bytes=by.value)

    def info(self):
        """dict(nbrows, nblocks, fwd_levels, bwd_levels, launches, form, us_per_level_launches, us_one_launch, factor_seconds,
        factor_bytes) — mi_bilu4_info."""
        nb, fl, bl, la, fo = (_c.c_int() for _ in range(5))
        nblk, by = _c.c_longlong(), _c.c_longlong()
        us = (_c.c_double * 2)()
        fs = _c.c_double()
        check(lib().mi_bilu4_info(self.handle, _c.byref(nb), _c.byref(nblk), _c.byref(fl), _c.byref(bl), _c.byref(la), _c.byref(fo), us,
                                  _c.byref(fs), _c.byref(by)))
        return dict(nbrows=nb.value, nblocks=nblk.value, fwd_levels=fl.value, bwd_levels=bl.value, launches=la.value, form=fo.value,
                    us_per_level_launches=us[0], us_one_launch=us[1], factor_seconds=fs.value, factor_bytes=by.value)

    def factor_host(self):
        """(ptr, col, diag, val): the host factor — val (nblocks, 4, 4) row-major: L multipliers, INVERTED diagonal blocks, U."""
        nblk = self.info()["nblocks"]
        ptr = np.zeros(self.nbrows + 1, np.int32)
        col = np.zeros(max(nblk, 1), np.int32)
        diag = np.zeros(max(self.nbrows, 1), np.int32)
        val = np.zeros((max(nblk, 1), 4, 4), np.float64)
        check(lib().mi_bilu4_factor_host(self.handle, ptr.ctypes.data, col.ctypes.data, diag.ctypes.data, val.ctypes.data, max(nblk, 1)))
        return ptr, col[:nblk], diag[: self.nbrows], val[:nblk]

BILU_ORDERS = ("natural", "colour")  # MI_BILU_ORDER_*


def _bilu_order(order):
    if order not in BILU_ORDERS:
        raise ValueError('bilu4: order must be "natural" or "colour"')
    return BILU_ORDERS.index(order)


def _sweep_precision(precision):
    """False for "f64", True for "f32"."""
    if precision not in ("f64", "f32"):
        raise ValueError('bilu4: precision must be "f64" or "f32"')
    return precision == "f32"


class bilu4_apply:
    """What bilu4.sweeps(fwd, bwd, precision) and bilu4.exact("f32") return: the factors of F applied by fixed numbers of Jacobi
    sweeps (sweeps=True) or exactly, over F's values (precision="f64") or their single-precision copy ("f32").  It shares F's handle
    and owns nothing."""

    def __init__(self, F, sweeps, precision="f64", fwd=0, bwd=0):
        self.F, self.sweeps, self.fwd, self.bwd, self.precision = F, bool(sweeps), int(fwd), int(bwd), precision
        self._way = _BILU_APPLY[self.sweeps, _sweep_precision(precision)]
        self._counts = (self.fwd, self.bwd) if self.sweeps else ()
        if self.fwd < 0 or self.bwd < 0:
            raise ValueError("bilu4.sweeps: negative sweep count")

    def solve(self, x, b):
        """x = this view's operator applied to b (see _bilu_solve for the vectors it takes)."""
        return _bilu_solve(self.F, self._way, self._counts, x, b)

    def gmres_args(self):
        return self.F.handle, self._way[2], self.fwd, self.bwd


def bilu4_sweeps(F, fwd, bwd, precision="f64"):
    return bilu4_apply(F, True, precision, fwd, bwd)


def bilu4_exact_f32(F):
    return bilu4_apply(F, False, "f32")


def bilu4_plan_probe(nbrows, ptrow, indcol, fill=0):
    """mi_bilu4_plan_probe (no GPU): dict(nblocks, fwd_levels, bwd_levels, fwd_launches, bwd_launches, fwd_sizes, bwd_sizes)."""
    ptrow = np.ascontiguousarray(ptrow, dtype=np.int32)
    indcol = np.ascontiguousarray(indcol, dtype=np.int32)
    nblk = _c.c_longlong()
    fl, bl, fa, ba = (_c.c_int() for _ in range(4))
    cap = max(int(nbrows), 1)
    fs, bs = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    check(lib().mi_bilu4_plan_probe(int(nbrows), ptrow.ctypes.data, indcol.ctypes.data, int(fill), _c.byref(nblk), _c.byref(fl), _c.byref(bl),
                                    _c.byref(fa), _c.byref(ba), fs.ctypes.data, bs.ctypes.data, cap))
    return dict(nblocks=nblk.value, fwd_levels=fl.value, bwd_levels=bl.value, fwd_launches=fa.value, bwd_launches=ba.value,
                fwd_sizes=fs[: fl.value].copy(), bwd_sizes=bs[: bl.value].copy())


def bilu4_order_probe(nbrows, ptrow, indcol, order="colour"):
    """mi_bilu4_order_probe (no GPU): dict(perm, ncolours, colour_sizes) of the ordering exactly as bilu4(..., order=) builds it, checked
    by the library before it is returned (MiError, status 6, naming the first violation)."""
    ptrow = np.ascontiguousarray(ptrow, dtype=np.int32)
    indcol = np.ascontiguousarray(indcol, dtype=np.int32)
    cap = max(int(nbrows), 1)
    perm, sizes, nc = np.zeros(cap, np.int32), np.zeros(cap, np.int32), _c.c_int()
    check(lib().mi_bilu4_order_probe(int(nbrows), ptrow.ctypes.data, indcol.ctypes.data if indcol.size else None, _bilu_order(order), perm.ctypes.data,
                                     _c.byref(nc), sizes.ctypes.data, cap))
    return dict(perm=perm[: int(nbrows)].copy(), ncolours=nc.value, colour_sizes=sizes[: nc.value].copy())


def bilu4dev_plan_probe(nbrows, ptrow, indcol, fill=0):
    """mi_bilu4dev_plan_probe (no GPU): dict(update_pairs, launches, plan_bytes) of the device refactor's plan."""
    ptrow = np.ascontiguousarray(ptrow, dtype=np.int32)
    indcol = np.ascontiguousarray(indcol, dtype=np.int32)
    up, by, la = _c.c_longlong(), _c.c_longlong(), _c.c_int()
    check(lib().mi_bilu4dev_plan_probe(int(nbrows), ptrow.ctypes.data, indcol.ctypes.data, int(fill), _c.byref(up), _c.byref(la), _c.byref(by)))
    return dict(update_pairs=up.value, launches=la.value, plan_bytes=by.value)


def dilu4dev_plan_probe(nbrows, ptrow, indcol, order="colour"):
    """mi_dilu4dev_plan_probe (no GPU): dict(pivot_pairs, launches, plan_bytes) of the block DILU's device refactor under `order`,
    built and checked by the library (MiError, status 6, naming the first violation)."""
    ptrow = np.ascontiguousarray(ptrow, dtype=np.int32)
    indcol = np.ascontiguousarray(indcol, dtype=np.int32)
    pp, by, la = _c.c_longlong(), _c.c_longlong(), _c.c_int()
    check(lib().mi_dilu4dev_plan_probe(int(nbrows), ptrow.ctypes.data, indcol.ctypes.data if indcol.size else None, _bilu_order(order), _c.byref(pp),
                                       _c.byref(la), _c.byref(by)))
    return dict(pivot_pairs=pp.value, launches=la.value, plan_bytes=by.value)


def bilu4one_plan_probe(nbrows, ptrow, indcol, fill=0, workgroups=0):
    """mi_bilu4one_plan_probe (no GPU): dict(eligible, why, nchunks, max_deps, plan_bytes, chunk_pos, chunk_lev, dep_ptr, dep) of the
    one-launch solve's plan, replayed for `workgroups` (0: 256); the last six are (forward, backward) pairs."""
    ptrow = np.ascontiguousarray(ptrow, dtype=np.int32)
    indcol = np.ascontiguousarray(indcol, dtype=np.int32)
    el, by = _c.c_int(), _c.c_longlong()
    nch, md = (_c.c_int * 2)(), (_c.c_int * 2)()
    args = (int(nbrows), ptrow.ctypes.data, indcol.ctypes.data if indcol.size else None, int(fill), int(workgroups))
    check(lib().mi_bilu4one_plan_probe(*args, _c.byref(el), nch, md, _c.byref(by), None, None, None, None))
    tabs = [[np.zeros(nch[b] + 1, np.int32) for b in range(2)] for _ in range(3)]
    ptrs = [(_c.c_void_p * 2)(t[0].ctypes.data, t[1].ctypes.data) for t in tabs]
    check(lib().mi_bilu4one_plan_probe(*args, _c.byref(el), nch, md, _c.byref(by), ptrs[0], ptrs[1], ptrs[2], None))
    dep = [np.zeros(max(int(tabs[2][b][-1]), 1), np.int32) for b in range(2)]
    dptr = (_c.c_void_p * 2)(dep[0].ctypes.data, dep[1].ctypes.data)
    check(lib().mi_bilu4one_plan_probe(*args, _c.byref(el), nch, md, _c.byref(by), None, None, None, dptr))
    why = "" if el.value else lib().mi_last_error().decode()
    return dict(eligible=bool(el.value), why=why, nchunks=(nch[0], nch[1]), max_deps=(md[0], md[1]), plan_bytes=by.value,
                chunk_pos=tuple(tabs[0]), chunk_lev=tuple(tabs[1]), dep_ptr=tuple(tabs[2]),
                dep=tuple(dep[b][: int(tabs[2][b][-1])] for b in range(2)))


RING_CENSUS = ("blocks table_len bpw runs_kind0 runs_kind1 runs_kind3 runs_nonempty runs_idle run_min run_max uniform lean depth "
               "runs_len1 runs_len2 runs_len3 runs_len4 runs_len5 runs_len9 "
               "runs_wide0 runs_wide1 runs_wide2 runs_wide3 runs_wide4 runs_wide5up wide_max_per_run "
               "plain plain_first plain_last plain_middle plain_after_plain plain_ends_matrix plain_long_row plain_span "
               "kind0_blocks kind0_wide kind0_long_row "
               "served served_full served_full_less1 served_row_limit served_rows_over_t served_span_ring served_span_max "
               "empty empty_first empty_last empty_middle restart_ahead restart_back restart_cold "
               "new_max new_below_t new_t new_t1 new_mid new_4t new_4t1 new_high new_ring slot_wrap base_advance").split()
MRING_CENSUS = ("blocks table_len runs table_padded runs_kind0 runs_kind1 runs_kind3 run_min run_max depth forced_cuts "
                "runs_wide0 runs_wide1 runs_wide2 runs_wide3 runs_wide4 runs_wide5up wide_max_per_run "
                "plain plain_first plain_last plain_middle plain_long_row plain_clusters plain_width kind0_blocks "
                "served served_clusters_k clusters_max served_width_limit width_max wide_clusters_k1 wide_width_limit1 "
                "gap_min_split gap_max_joined empty "
                "groups_max groups_full group_ends_at_wrap group_starts_at_wrap block_across_wrap group_past_end first_past_end").split()


def ring_plan_census(n, ptrow, indcol, config_id):
    """mi_ring_plan_census (no GPU): dict of the counters include/mi355_spmv.h lists, by the names of RING_CENSUS."""
    ptrow = np.ascontiguousarray(ptrow, np.int32)
    indcol = np.ascontiguousarray(indcol, np.int32)
    out = np.zeros(len(RING_CENSUS), np.int64)
    check(lib().mi_ring_plan_census(int(n), ptrow.ctypes.data, indcol.ctypes.data if indcol.size else None, int(config_id), out.ctypes.data, out.size))
    return dict(zip(RING_CENSUS, out.tolist()))


def mring_plan_census(n, ptrow, indcol):
    """mi_mring_plan_census (no GPU): dict of the counters include/mi355_spmv.h lists, by the names of MRING_CENSUS."""
    ptrow = np.ascontiguousarray(ptrow, np.int32)
    indcol = np.ascontiguousarray(indcol, np.int32)
    out = np.zeros(len(MRING_CENSUS), np.int64)
    check(lib().mi_mring_plan_census(int(n), ptrow.ctypes.data, indcol.ctypes.data if indcol.size else None, out.ctypes.data, out.size))
    return dict(zip(MRING_CENSUS, out.tolist()))


ROWBLOCK_CENSUS = ("blocks row_align idle_wgs empty empty_first empty_last empty_middle "
                   "full full_less1 nn_mod8_1 nn_mod8_7 nn_1 "
                   "rows_1 rows_t rows_t1 rows_cap rows_max ended_by_cap pulled_back "
                   "first_row_empty last_row_empty rowlen_1 rowlen_8 rowlen_9 "
                   "long long_plus1 long_2x long_2x1 long_first_row long_last_row long_after_long "
                   "r1 r2 r3 r4 r5 r6 r7 r8 u_1 u_mult u_mult1 u_eq_nn u_max skew").split()


def rowblock_census(n, ptrow, indcol, which, starts=False):
    """mi_rowblock_census (no GPU): dict of the counters include/mi355_spmv.h lists, by the names of ROWBLOCK_CENSUS, for the row
    blocks of the stream kernel (which = "stream") or the tile kernel's plan ("tile").  starts=True: (dict, first row of every
    block followed by n)."""
    ptrow = np.ascontiguousarray(ptrow, np.int32)
    indcol = np.ascontiguousarray(indcol, np.int32)
    k = len(ROWBLOCK_CENSUS)
    out = np.zeros(k + (int(n) + 1 if starts else 0), np.int64)
    check(lib().mi_rowblock_census(int(n), ptrow.ctypes.data, indcol.ctypes.data if indcol.size else None, KERNELS[which], out.ctypes.data, out.size))
    S = dict(zip(ROWBLOCK_CENSUS, out[:k].tolist()))
    return (S, out[k:k + S["blocks"] + 1].copy()) if starts else S


def bcsr4_tile_probe(nbrows, ptrow, indcol):
    """mi_bcsr4_tile_probe (no GPU): dict(would_build, groups, max_nodes, groups_at_cap) — the x-tile lists of the blocked kernel."""
    ptrow = np.ascontiguousarray(ptrow, np.int32)
    indcol = np.ascontiguousarray(indcol, np.int32)
    v = [_c.c_int() for _ in range(4)]
    check(lib().mi_bcsr4_tile_probe(int(nbrows), ptrow.ctypes.data, indcol.ctypes.data if indcol.size else None, *[_c.byref(t) for t in v]))
    return dict(would_build=bool(v[0].value), groups=v[1].value, max_nodes=v[2].value, groups_at_cap=v[3].value)


def spmk_plan_probe(n, ptrow, indcol):
    """mi_spmk_plan_probe (no GPU): (eligible, runs, max_deps) of the one-launch powers step's plan, checked in C++."""
    ptrow = np.ascontiguousarray(ptrow, dtype=np.int32)
    indcol = np.ascontiguousarray(indcol, dtype=np.int32)
    e, r, m = _c.c_int(), _c.c_int(), _c.c_int()
    check(lib().mi_spmk_plan_probe(int(n), ptrow.ctypes.data, indcol.ctypes.data if indcol.size else None, _c.byref(e), _c.byref(r), _c.byref(m)))
    return bool(e.value), r.value, m.value


def spmk_plan_dump(n, ptrow, indcol):
    """mi_spmk_plan_dump (no GPU): dict(T, nblk, wgs, bpw, uniform, in_loop, lean, plan (nblk, 8), run_rng (wgs, 2), dep_ptr
    (wgs + 1), dep_run) — ring configuration 4's plan and the one-launch powers step's dependency lists as mi_csr_create builds them."""
    ptrow = np.ascontiguousarray(ptrow, dtype=np.int32)
    indcol = np.ascontiguousarray(indcol, dtype=np.int32)
    info = np.zeros(8, np.int32)
    args = (int(n), ptrow.ctypes.data, indcol.ctypes.data if indcol.size else None, info.ctypes.data)
    check(lib().mi_spmk_plan_dump(*args, None, None, None, None, 0, 0, 0))
    T, nblk, wgs, bpw, uniform, in_loop, ndep, lean = (int(t) for t in info)
    plan = np.zeros((max(nblk, 1), 8), np.int32)
    rng = np.zeros((max(wgs, 1), 2), np.int32)
    dptr = np.zeros(wgs + 1, np.int32)
    drun = np.zeros(max(ndep, 1), np.int32)
    check(lib().mi_spmk_plan_dump(*args, plan.ctypes.data, rng.ctypes.data, dptr.ctypes.data, drun.ctypes.data, nblk, wgs, ndep))
    return dict(T=T, nblk=nblk, wgs=wgs, bpw=bpw, uniform=bool(uniform), in_loop=bool(in_loop), lean=bool(lean), plan=plan[:nblk],
                run_rng=rng[:wgs], dep_ptr=dptr, dep_run=drun[:ndep])


def bcsr4_sell_plan_probe(nbrows, ptrow, indcol, nwaves_max=1024):
    """mi_bcsr4_sell_plan_probe (no GPU): dict(nslices, nsteps, nwaves, sptr, wrng, col) — the slice table of the blocked kernel's
    sliced copy; sptr has nslices + 3 entries, wrng nwaves + 1, col (nsteps + 48, 16) as uint32."""
    ptrow = np.ascontiguousarray(ptrow, dtype=np.int32)
    indcol = np.ascontiguousarray(indcol, dtype=np.int32)
    ns, nw, st = _c.c_int(), _c.c_int(), _c.c_longlong()
    args = (int(nbrows), ptrow.ctypes.data, indcol.ctypes.data if indcol.size else None, int(nwaves_max))
    check(lib().mi_bcsr4_sell_plan_probe(*args, _c.byref(ns), _c.byref(st), _c.byref(nw), None, None, None))
    sptr, wrng = np.zeros(ns.value + 3, np.int32), np.zeros(nw.value + 1, np.int32)
    col = np.zeros((st.value + 48, 16), np.uint32)
    check(lib().mi_bcsr4_sell_plan_probe(*args, _c.byref(ns), _c.byref(st), _c.byref(nw), sptr.ctypes.data, wrng.ctypes.data, col.ctypes.data))
    return dict(nslices=ns.value, nsteps=st.value, nwaves=nw.value, sptr=sptr, wrng=wrng, col=col)


def bcsr4_spmm_plan_probe(nbrows, ptrow, indcol, per=128, ucap=None):
    """mi_bcsr4_spmm_plan_probe (no GPU): the tile plan of the multi-vector product's forms 1 (per = 128) and 2, 3 (per = 64) —
    dict(refused, per, ntiles, umax, mean_list, wg_ptr, nodes, slots, rows): wg_ptr has ntiles + 1 entries, nodes wg_ptr[-1] (the pad
    entry dropped), slots one per block (uint16; the pad entry dropped), rows (ntiles, per).  ucap None: the handle's default cap."""
    ptrow = np.ascontiguousarray(ptrow, dtype=np.int32)
    indcol = np.ascontiguousarray(indcol, dtype=np.int32)
    nbrows, per = int(nbrows), int(per)
    if ucap is None:
        ucap = 368 if per == 128 else 256
    nb = int(ptrow[nbrows]) if nbrows > 0 else 0
    ref, nt, um, ml = _c.c_int(), _c.c_int(), _c.c_int(), _c.c_double()
    wg, nodes = np.zeros(nbrows + 1, np.int32), np.zeros(nb + 1, np.uint32)
    slots, rows = np.zeros(nb + 1, np.uint16), np.zeros(max(nbrows * per, 1), np.int32)
    check(lib().mi_bcsr4_spmm_plan_probe(nbrows, ptrow.ctypes.data, indcol.ctypes.data if indcol.size else None, per, int(ucap), _c.byref(ref),
                                         _c.byref(nt), _c.byref(um), _c.byref(ml), wg.ctypes.data, wg.size, nodes.ctypes.data, nodes.size,
                                         slots.ctypes.data, slots.size, rows.ctypes.data, rows.size))
    out = dict(refused=bool(ref.value), per=per, ntiles=nt.value, umax=um.value, mean_list=ml.value)
    if not out["refused"]:
        wg = wg[: nt.value + 1].copy()
        out.update(wg_ptr=wg, nodes=nodes[: wg[-1]].copy(), slots=slots[:nb].copy(), rows=rows[: nt.value * per].reshape(nt.value, per).copy())
    return out


def MatSolve_SeqBAIJ_4(F, b, x):
    """x = U^-1 L^-1 b with the factors F (a bilu4) — MatSolve_SeqBAIJ_4(A, bb, xx), src/kernels/baij4_solve.c:4-93."""
    return F.solve(x, b)


class dilu4(_OwnsHandle):
    """mi_dilu4_t: the block DILU preconditioner M = (E + L) E^-1 (E + U) of a square 4x4-block matrix B = L + D + U, applied with
    Eisenstat's trick: apply_hat is the split-preconditioned operator A^ = (E + L)^-1 B (E + U)^-1 E at the cost of ONE backward and
    ONE forward triangular sweep, with no separate product (include/mi355_spmv.h, mi_dilu4_*).  dilu4(A, order="colour") takes a
    bcsr4x4_matrix's host arrays (and its block layout); dilu4(nbrows, ptrow, indcol, coef, layout="row") the arrays themselves.
    order: "colour" (the multicolour ordering of bilu4, where DILU measured as good as ILU(0)) or "natural"; every method keeps the
    caller's numbering.  host_only=True: no device copy (refactor, fetch, info only).  Opt-in: nothing chooses it.  The three
    operations take CUDA tensors, run asynchronously on torch's current stream, allocate nothing and may run in place; one operation
    at a time per handle.  New values on the same pattern: refactor(coef) from the host (waits, uploads) or refactor_dev(coef) from a
    CUDA tensor, on the GPU and on the current stream (mi_dilu4dev_*; the same bits)."""

    _destroy = "mi_dilu4_destroy"

    def __init__(self, A, ptrow=None, indcol=None, coef=None, layout="row", host_only=False, order="colour"):
        self.nbrows, ptrow, indcol, coef, lay = _block_pattern(A, ptrow, indcol, coef, layout)
        self.layout = lay
        self.order = order
        self._nblocks_in = len(indcol)
        h = _vp()
        make = lib().mi_dilu4_create_host if host_only else lib().mi_dilu4_create
        check(make(self.nbrows, ptrow.ctypes.data, indcol.ctypes.data, coef.ctypes.data, lay, _bilu_order(order), _c.byref(h)))
        self._h = h

    def _sweep(self, fn, out, src):
        n = 4 * self.nbrows
        check(fn(self.handle, _dev_ptr(src, n, "input"), _dev_ptr(out, n, "output"), _stream_ptr()))
        return out

    def to_hat(self, bhat, r):
        """bhat = (E + L)^-1 r (mi_dilu4_to_hat_dev); bhat may be r."""
        return self._sweep(lib().mi_dilu4_to_hat_dev, bhat, r)

    def from_hat(self, x, u):
        """x = (E + U)^-1 E u (mi_dilu4_from_hat_dev); x may be u."""
        return self._sweep(lib().mi_dilu4_from_hat_dev, x, u)

    def apply_hat(self, w, u):
        """w = A^ u = (E + L)^-1 B (E + U)^-1 E u (mi_dilu4_apply_hat_dev); w may be u."""
        return self._sweep(lib().mi_dilu4_apply_hat_dev, w, u)

    def refactor(self, coef):
        """New values on the same pattern (host array, the layout of construction): the pivots are recomputed on the host and
        uploaded (mi_dilu4_refactor; waits for the device)."""
        coef = _host_f64(coef, 16 * self._nblocks_in, "coef")
        check(lib().mi_dilu4_refactor(self.handle, coef.ctypes.data, self.layout))
        return self

    def prepare_dev(self):
        """Build, check and upload the pattern-only tables of the device refactor (mi_dilu4dev_prepare; idempotent)."""
        check(lib().mi_dilu4dev_prepare(self.handle))
        return self

    def refactor_dev(self, coef):
        """New values on the same pattern from a CUDA tensor (the block order and layout of construction): both triangles, Einv
        and K are rewritten on the GPU, asynchronously on torch's current stream (mi_dilu4dev_refactor; capturable once prepared).
        A refused pivot shows in factor_status(); fetch() follows only after fetch_dev()."""
        check(lib().mi_dilu4dev_refactor(self.handle, _dev_ptr(coef, 16 * self._nblocks_in, "coef"), self.layout, _stream_ptr()))
        return self

    def factor_status(self):
        """Wait for the last refactor_dev; MiError (MI_ERR_ARG, naming the caller's block row) when it refused a pivot."""
        bad = _c.c_int()
        check(lib().mi_dilu4dev_status(self.handle, _c.byref(bad)))
        return self

    def fetch_dev(self):
        """Copy the device's triangles, Einv and K back into the host copies, so that fetch() returns what the device holds
        (mi_dilu4dev_fetch; waits)."""
        check(lib().mi_dilu4dev_fetch(self.handle))
        return self

    def info_dev(self):
        """dict(prepared, launches, plan_bytes) — mi_dilu4dev_info; launches: of one refactor_dev."""
        pr, la, by = _c.c_int(), _c.c_int(), _c.c_longlong()
        check(lib().mi_dilu4dev_info(self.handle, _c.byref(pr), _c.byref(la), _c.byref(by)))
        return dict(prepared=bool(pr.value), launches=la.value, plan_bytes=by.value)

    def fetch(self):
        """(Einv, K), each (nbrows, 4, 4) row-major by the caller's block row (mi_dilu4_fetch): the inverted pivots and 2E - D."""
        einv = np.zeros((max(self.nbrows, 1), 4, 4))
        k = np.zeros((max(self.nbrows, 1), 4, 4))
        check(lib().mi_dilu4_fetch(self.handle, einv.ctypes.data, k.ctypes.data))
        return einv[: self.nbrows], k[: self.nbrows]

    def info(self):
        """dict(nbrows, nblocks, order, ncolours, fwd_levels, bwd_levels, launches, factor_seconds, device_bytes, perm) —
        mi_dilu4_info; launches: of one apply_hat; perm[caller's block row] = the row of B."""
        nb, o, nc, fl, bl, la = (_c.c_int() for _ in range(6))
        nblk, by = _c.c_longlong(), _c.c_longlong()
        fs = _c.c_double()
        perm = np.zeros(max(self.nbrows, 1), np.int32)
        check(lib().mi_dilu4_info(self.handle, _c.byref(nb), _c.byref(nblk), _c.byref(o), _c.byref(nc), _c.byref(fl), _c.byref(bl), _c.byref(la),
                                  _c.byref(fs), _c.byref(by), perm.ctypes.data))
        return dict(nbrows=nb.value, nblocks=nblk.value, order=BILU_ORDERS[o.value], ncolours=nc.value, fwd_levels=fl.value,
                    bwd_levels=bl.value, launches=la.value, factor_seconds=fs.value, device_bytes=by.value, perm=perm[: self.nbrows])

    def gmres(self, A, b, x, restart=30, rtol=1e-8, maxiter=300, check_every=None, basis="f64"):
        """Solve A x = b (A: the bcsr4x4_matrix this handle was made from; b, x CUDA tensors, x the initial guess, then the solution)
        by GMRES on the split-preconditioned system: r = b - A x0 (the one true product), b^ = to_hat(r), u^ = 0, A^ u^ = b^ with
        gmres_solver(self), x = x0 + from_hat(u^).  (iterations, history, reason) of that solve: rtol AND THE HISTORY ARE IN THE HAT
        NORM, ||(E + L)^-1 r|| / ||b^||, not in the norm of b - A x."""
        import torch

        w = torch.empty_like(b)
        SpMV_BCSR(w, x, A)
        r = b.clone()
        axpy(-1.0, w, r)
        self.to_hat(r, r)
        u = torch.zeros_like(b)
        S = gmres_solver(self, None, restart, basis)
        try:
            out = S.solve(r, u, rtol=rtol, maxiter=maxiter, check_every=GMRES_CHECK_EVERY if check_every is None else check_every)
            self.from_hat(u, u)
            axpy(1.0, u, x)
            torch.cuda.current_stream().synchronize()  # (the solver and the work vectors go out of scope)
        finally:
            S.close()
        return out

class DistVector:
    """mi_dist_vec_t: a vector distributed like the rows of a DistMatrix (per rank [owned | halo] on the rank's device)."""

    def __init__(self, D, host=None):
        self.D = D
        h = _vp()
        check(lib().mi_dist_vec_create(D.handle, _c.byref(h)))
        self._h = h
        if host is not None:
            self.set(host)

    def set(self, host):
        host = _host_f64(host, self.D.n, "x")
        check(lib().mi_dist_vec_set(self._h, host.ctypes.data))
        return self

    def get(self, out=None):
        out = np.empty(self.D.n, np.float64) if out is None else _host_f64(out, self.D.n, "out", writable=True)
        check(lib().mi_dist_vec_get(self._h, out.ctypes.data))
        return out

    def close(self):
        if self._h is not None:  # (safe after its DistMatrix is closed: mi_dist_destroy released the device memory, this frees the host object)
            lib().mi_dist_vec_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DistMatrix:
    """mi_dist_t (include/mi355_spmv.h): one csrmatrix row-partitioned over `ndev` GPUs behind ONE handle of ONE process — the
    form of the multi-GPU path the reference's single-process harnesses reach (SpMV_CSR / SpM4V / orthogonalize of mpk/SpMV.h
    through the shim with MI355_NGPUS).  Host vectors: spmv / spmk / dot / orthogonalize mirror the reference's calls;
    device-resident vectors: vector(), spmv_dev / spmk_dev / synchronize."""

    def __init__(self, ndev, n, ptrow, indcol, coef):
        self.ndev, self.n = int(ndev), int(n)
        ptrow = np.ascontiguousarray(ptrow, dtype=np.int32)
        indcol = np.ascontiguousarray(indcol, dtype=np.int32)
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        self.nnz = int(ptrow[-1]) if self.n > 0 else 0
        h = _vp()
        self._h = None
        check(lib().mi_dist_create(self.ndev, self.n, ptrow.ctypes.data, indcol.ctypes.data, coef.ctypes.data, _c.byref(h)))
        self._h = h

    @property
    def handle(self):
        return self._h

    def info(self):
        L = lib()
        nr, dd, ex, fu, ht, hm = _c.c_int(), _c.c_int(), _c.c_int(), _c.c_int(), _c.c_longlong(), _c.c_longlong()
        check(L.mi_dist_info(self._h, _c.byref(nr), _c.byref(dd), _c.byref(ex), _c.byref(fu), _c.byref(ht), _c.byref(hm)))
        ranks = []
        for r in range(nr.value):
            dev, r0, nl, nh, nz, st = _c.c_int(), _c.c_longlong(), _c.c_int(), _c.c_int(), _c.c_longlong(), _vp()
            check(L.mi_dist_rank_info(self._h, r, _c.byref(dev), _c.byref(r0), _c.byref(nl), _c.byref(nh), _c.byref(nz), _c.byref(st)))
            ranks.append(dict(device=dev.value, row_start=r0.value, n_local=nl.value, n_halo=nh.value, nnz_local=nz.value))
        return dict(nranks=nr.value, distinct_devices=dd.value, exchange=L.mi_dist_exchange_name(self._h).decode(),
                    fused=bool(fu.value), halo_total=ht.value, halo_max=hm.value, note=L.mi_dist_exchange_note(self._h).decode(),
                    ranks=ranks)

    def update_values(self, coef):
        coef = _host_f64(coef, self.nnz, "coef")
        check(lib().mi_dist_update_values(self._h, coef.ctypes.data))

    # -- host vectors: the reference's calling convention
    def spmv(self, y, x):
        x, y = _host_f64(x, self.n, "x"), _host_f64(y, self.n, "y", writable=True)
        check(lib().mi_dist_spmv(self._h, x.ctypes.data, y.ctypes.data))
        return y

    def spmk(self, ys, x):
        x = _host_f64(x, self.n, "x")
        ys = [_host_f64(t, self.n, "y_out", writable=True) for t in ys]
        arr = (_vp * len(ys))(*[t.ctypes.data for t in ys])
        check(lib().mi_dist_spmk(self._h, len(ys), x.ctypes.data, arr))
        return ys

    def dot(self, x, y):
        out = _c.c_double()
        check(lib().mi_dist_dot(self._h, _host_f64(x, self.n).ctypes.data, _host_f64(y, self.n).ctypes.data, _c.byref(out)))
        return out.value

    def orthogonalize(self, b, x1, x3, alpha=1e-8):
        beta = _c.c_double()
        x3 = _host_f64(x3, self.n, "x3", writable=True)
        check(lib().mi_dist_orthogonalize(self._h, _host_f64(b, self.n).ctypes.data, _host_f64(x1, self.n).ctypes.data, x3.ctypes.data,
                                          float(alpha), _c.byref(beta)))
        return beta.value

    # -- device-resident vectors
    def vector(self, host=None):
        return DistVector(self, host)

    def spmv_dev(self, y, x):
        check(lib().mi_dist_spmv_dev(self._h, x._h, y._h))

    def spmk_dev(self, ys, x):
        arr = (_vp * len(ys))(*[t._h for t in ys])
        check(lib().mi_dist_spmk_dev(self._h, len(ys), x._h, arr))

    def dot_dev(self, a, b):
        out = _c.c_double()
        check(lib().mi_dist_dot_dev(self._h, a._h, b._h, _c.byref(out)))
        return out.value

    def orthogonalize_dev(self, b, x1, x3, alpha=1e-8, want_beta=True):
        """x3 = x1 - alpha (b . x1) b on distributed vectors.  want_beta=False: nothing is awaited (the ranks' partial dots meet on the
        devices; returns None); else the call waits for rank 0's copy of beta and returns it."""
        if not want_beta:
            check(lib().mi_dist_orthogonalize_dev(self._h, b._h, x1._h, x3._h, float(alpha), None))
            return None
        beta = _c.c_double()
        check(lib().mi_dist_orthogonalize_dev(self._h, b._h, x1._h, x3._h, float(alpha), _c.byref(beta)))
        return beta.value

    def synchronize(self):
        check(lib().mi_dist_synchronize(self._h))

    def close(self):
        if self._h is not None:
            lib().mi_dist_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def COO2CSR(nrow, irow, jcol, val):
    """COO -> csrmatrix with the reference's rules (mpk/utils.cpp:5-43, :97-127):
    columns ascending per row, the FIRST of duplicated (i, j) entries wins.
    Host-side integer work (numpy): a stable sort on (row, col) keeps COO order
    among duplicates, so the first survivor of each run is the first COO entry."""
    irow = np.asarray(irow, dtype=np.int64)
    jcol = np.asarray(jcol, dtype=np.int64)
    val = np.asarray(val, dtype=np.float64)
    order = np.lexsort((np.arange(len(irow)), jcol, irow))
    r, c, v = irow[order], jcol[order], val[order]
    keep = np.ones(len(r), bool)
    keep[1:] = (r[1:] != r[:-1]) | (c[1:] != c[:-1])
    r, c, v = r[keep], c[keep], v[keep]
    ptrow = np.zeros(nrow + 1, np.int64)
    np.add.at(ptrow, r + 1, 1)
    ptrow = np.cumsum(ptrow)
    return csrmatrix(nrow, ptrow.astype(np.int32), c.astype(np.int32), v)


class _PlacedBuffer:
    """A device vector allocated by mi_vec_alloc_placed, visible to torch through __cuda_array_interface__."""

    def __init__(self, ptr, n):
        self.ptr = ptr
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (ptr, False), "version": 2, "strides": None}

    def __del__(self):
        try:
            if self.ptr:
                lib().mi_vec_free_placed(self.ptr)
                self.ptr = 0
        except Exception:
            pass


# --------------------------------------------------------------------- SpMV

def SpMV_CSR(y, x, A):
    """y = A x — SpMV_CSR(double* y, double* x, csrmatrix& A), mpk/SpMV.cpp:6-20.
    y is fully overwritten.  Tensors on the GPU: asynchronous on torch's current
    stream; numpy arrays: copied in/out and synchronised."""
    if _is_torch(x):
        check(lib().mi_spmv_dev(A.handle, _dev_ptr(x, A.ncols, "x"), _dev_ptr(y, A.n if A.rowmap is None else None, "y"),
                                _stream_ptr()))
    else:
        xx = _host_f64(x, A.ncols, "x")
        yy = _host_f64(y, A.n, "y", writable=True)
        check(lib().mi_spmv(A.handle, xx.ctypes.data, yy.ctypes.data))
    return y


def SpMV_CSR_internal(y_int, x_int, A):
    """y_int = A x_int with both vectors in the library's numbering (csrmatrix.to_internal / from_internal): what a Krylov
    loop calls between its one permutation in and its one permutation out.  Device tensors only."""
    check(lib().mi_spmv_internal_dev(A.handle, _dev_ptr(x_int, A.n, "x_int"), _dev_ptr(y_int, A.n, "y_int"), _stream_ptr()))
    return y_int


# The reference's four CSR variants differ only in how the CPU is driven
# (scalar / compiler FMA / __builtin_fma / AVX2, mpk/SpMV.cpp:23-85); on the GPU
# they are one kernel, bit-equal to _OPT/_FMA.
SpMV_CSR_OPT = SpMV_CSR
SpMV_CSR_FMA = SpMV_CSR
SpMV_CSR_AVX2 = SpMV_CSR


def SpMV_BCSR(y, x, A):
    """y = A x for bcsr4x4_matrix — SpMV_BCSR*, mpk/SpMV.cpp:90-219."""
    if _is_torch(x):
        check(lib().mi_bcsr4_spmv_dev(A.handle, _dev_ptr(x, 4 * A.nbcols, "x"), _dev_ptr(y, 4 * A.nrows, "y"), _stream_ptr()))
    else:
        xx = _host_f64(x, None, "x")
        if xx.size < 4 * A.nbcols:  # the reference reads x by block column; pad like its callers' vectors
            xx = np.concatenate([xx, np.zeros(4 * A.nbcols - xx.size)])
        yy = _host_f64(y, 4 * A.nrows, "y", writable=True)
        check(lib().mi_bcsr4_spmv(A.handle, xx.ctypes.data, yy.ctypes.data))
    return y


SpMV_BCSR_OPT = SpMV_BCSR
SpMV_BCSR_FMA = SpMV_BCSR
SpMV_BCSR_AVX2 = SpMV_BCSR


# ------------------------------------------------------------ matrix powers

def SpMkV(ys, x, A):
    """ys[p] = A^(p+1) x for p = 0..k-1 (all intermediate powers, as SpM4V returns them)."""
    k = len(ys)
    if _is_torch(x):
        ptrs = (_vp * k)(*[_dev_ptr(t, A.n, f"y{p + 1}").value for p, t in enumerate(ys)])
        check(lib().mi_spmk_dev(A.handle, k, _dev_ptr(x, A.ncols, "x"), ptrs, _stream_ptr()))
    else:
        xx = _host_f64(x, A.ncols, "x")
        outs = [_host_f64(t, A.n, f"y{p + 1}", writable=True) for p, t in enumerate(ys)]
        ptrs = (_vp * k)(*[o.ctypes.data for o in outs])
        check(lib().mi_spmk(A.handle, k, xx.ctypes.data, ptrs))
    return ys


def Generate1stlayer(ptrowend1, A):
    """mpk/SpM2V.cpp:5-26: ptrowend1[ia] = ptrow[j + 1] the first time column j = indcol[ia] is met in
    CSR traversal order, else ptrow[j].  The table drives the CPU's serial traversal; the GPU path does
    not need it (each power is a full row-parallel sweep) but callers may inspect it, so it is filled
    as the reference fills it.  ptrowend1: int32 array of >= nnz entries (or None: a new one)."""
    nnz = A.nnz
    if ptrowend1 is None:
        ptrowend1 = np.zeros(nnz, np.int32)
    cols = A.indcol[:nnz].astype(np.int64)
    ptrowend1[:nnz] = A.ptrow[cols]
    _, first = np.unique(cols, return_index=True)
    ptrowend1[first] = A.ptrow[cols[first] + 1]
    return ptrowend1


def SpM2V_CSR(z, y, x, A, ptrowend1=None):
    """y = A x, z = A (A x) — SpM2V_CSR(z, y, x, A, ptrowend1), mpk/SpM2V.cpp:79-112."""
    SpMkV([y, z], x, A)
    return z, y


SpM2V_CSR_OPT = SpM2V_CSR
SpM2V_CSR_FMA = SpM2V_CSR
SpM2V_CSR_AVX2 = SpM2V_CSR


def SpM3V(w, z, y, x, A, ptrowend1=None, ptrowend2=None):
    """mpk/SpMVmulti0.cpp:132-155."""
    SpMkV([y, z, w], x, A)
    return w, z, y


def SpM4V(v, w, z, y, x, A, ptrowend1=None, ptrowend2=None, ptrowend3=None):
    """y=Ax, z=A^2x, w=A^3x, v=A^4x — SpM4V(v, w, z, y, x, A, ...), mpk/SpMVmulti0.cpp:189-221."""
    SpMkV([y, z, w, v], x, A)
    return v, w, z, y


def SpM2V_BCSR(z, y, x, A, ptrowend1=None):
    """y = A x, z = A (A x) on a bcsr4x4_matrix — SpM2V_BCSR{,_OPT,_FMA,_AVX2}(z, y, x, A, ptrowend1),
    mpk/SpM2V.cpp:375-801 (square matrices)."""
    n = 4 * A.nrows
    if _is_torch(x):
        ptrs = (_vp * 2)(_dev_ptr(y, n, "y").value, _dev_ptr(z, n, "z").value)
        check(lib().mi_bcsr4_spmk_dev(A.handle, 2, _dev_ptr(x, n, "x"), ptrs, _stream_ptr()))
    else:
        yy, zz = _host_f64(y, n, "y", writable=True), _host_f64(z, n, "z", writable=True)
        ptrs = (_vp * 2)(yy.ctypes.data, zz.ctypes.data)
        check(lib().mi_bcsr4_spmk(A.handle, 2, _host_f64(x, n, "x").ctypes.data, ptrs))
    return z, y


SpM2V_BCSR_OPT = SpM2V_BCSR
SpM2V_BCSR_FMA = SpM2V_BCSR
SpM2V_BCSR_AVX2 = SpM2V_BCSR


# ------------------------------------------------- multi-vector products, Krylov basis

ARITH = {"chain": 0, "blockacc": 1}


def MatMatMult_SeqBAIJ_4(A, X, Y, arith="chain"):
    """Y[:, j] = A X[:, j] for the s columns of X with the matrix read once — MatMatMult_SeqBAIJ_4_AVX2(A, X, Y, s_step),
    src/kernels/spmm_avx2.c:7-109.  A: bcsr4x4_matrix (any arith) or csrmatrix (chain).  X, Y: column-major (n, s): CUDA
    tensors of shape (s, n) (row j = column j, as MatDense stores it) or numpy arrays of shape (s, n)."""
    s = int(X.shape[0])
    if isinstance(A, csrmatrix):
        assert arith == "chain"
        check(lib().mi_spmm_dev(A.handle, s, _dev_ptr(X), int(X.stride(0)), _dev_ptr(Y), int(Y.stride(0)), _stream_ptr()))
        return Y
    if _is_torch(X):
        check(lib().mi_bcsr4_spmm_dev(A.handle, s, _dev_ptr(X), int(X.stride(0)), _dev_ptr(Y), int(Y.stride(0)), ARITH[arith], _stream_ptr()))
    else:
        XX = np.ascontiguousarray(X, dtype=np.float64)
        assert isinstance(Y, np.ndarray) and Y.flags.c_contiguous and Y.dtype == np.float64
        check(lib().mi_bcsr4_spmm(A.handle, s, XX.ctypes.data, XX.shape[1], Y.ctypes.data, Y.shape[1], ARITH[arith]))
    return Y


def BuildKrylovBasis(A, v0, s, orth=False):
    """orth=False: V[0] = v0, V[k+1] = A V[k], k < s — BuildKrylovBasis_AVX2, src/kernels/spmm_avx2.c:112-168.
    orth=True: the orthonormal (Arnoldi) basis of the same space (mi_krylov_basis_dev explains).
    orth="cgs" / "cgs2": the same basis by classical Gram-Schmidt with one / two passes (mi_krylov_basis_cgs_dev); "cgs2"
    stays orthonormal where the other two do not.  Returns (V, H, nrm0):
    V a CUDA tensor of shape (s+1, n) (row k = basis vector k); H (s, s+2) with H[k, :k+1] the dots of step k and
    H[k, k+1] the norm, nrm0 = ||v0|| (both None when orth is False)."""
    import torch
    if isinstance(orth, str) and orth not in ("cgs", "cgs2"):
        raise ValueError(f"orth: expected False, True, 'cgs' or 'cgs2', got {orth!r}")
    n = A.n
    V = torch.empty((s + 1, n), dtype=torch.float64, device="cuda")
    coef = torch.zeros(s * (s + 2) + 1, dtype=torch.float64, device="cuda") if orth else None
    if isinstance(orth, str):
        check(lib().mi_krylov_basis_cgs_dev(A.handle, s, _dev_ptr(v0, n), _dev_ptr(V), n, 2 if orth == "cgs2" else 1,
                                            _dev_ptr(coef), _stream_ptr()))
    else:
        check(lib().mi_krylov_basis_dev(A.handle, s, _dev_ptr(v0, n), _dev_ptr(V), n, 1 if orth else 0,
                                        _dev_ptr(coef) if orth else None, _stream_ptr()))
    if not orth:
        return V, None, None
    return V, coef[: s * (s + 2)].reshape(s, s + 2), coef[s * (s + 2)]


def GMRES(A, b, x, M=None, restart=30, rtol=1e-8, maxiter=300):
    """Right-preconditioned restarted GMRES, KSPGMRES with restart 30 of src/solve_newton.c:1156-1164, assembled from the
    library's pieces: the product (SpMV_BCSR / SpMV_CSR), classical Gram-Schmidt with two passes (cgs: VecMDot / VecMAXPY),
    maxpy for the update and, with M (a bilu4), MatSolve_SeqBAIJ_4 as the preconditioner: A M^-1 u = b, x = x0 + M^-1 u.
    b, x: CUDA tensors; x holds the initial guess and receives the solution.  The small Hessenberg least-squares problem is
    solved on the host (Givens rotations), with one read-back of h per iteration.  Stops when the recurrence's relative
    residual ||r|| / ||b|| <= rtol or after maxiter iterations.  Returns (iterations, history): history[0] the true relative
    residual of the initial guess, then one entry per iteration (the recurrence's value; a restart recomputes the true one)."""
    import torch
    mult = SpMV_BCSR if isinstance(A, bcsr4x4_matrix) else SpMV_CSR
    n = int(b.numel())
    V = torch.empty((restart + 1, n), dtype=torch.float64, device=b.device)
    w, z = torch.empty_like(b), torch.empty_like(b)
    bnorm = float(norm2(b).item()) or 1.0
    its, hist = 0, []
    while True:
        mult(w, x, A)
        r = V[0]
        r.copy_(b)
        axpy(-1.0, w, r)
        beta = float(norm2(r).item())
        if not hist:
            hist.append(beta / bnorm)
        if beta / bnorm <= rtol or its >= maxiter or not np.isfinite(beta):
            return its, hist
        r.mul_(1.0 / beta)
        H = np.zeros((restart + 1, restart))
        cs, sn, g = np.zeros(restart), np.zeros(restart), np.zeros(restart + 1)
        g[0] = beta
        k = 0
        while k < restart and its < maxiter:
            if M is not None:
                M.solve(z, V[k])
                mult(w, z, A)
            else:
                mult(w, V[k], A)
            h, nrm = cgs([V[j] for j in range(k + 1)], w, passes=2)
            hk = torch.cat([h, nrm]).cpu().numpy()  # the iteration's one read-back
            H[: k + 2, k] = hk
            for j in range(k):
                t = cs[j] * H[j, k] + sn[j] * H[j + 1, k]
                H[j + 1, k] = -sn[j] * H[j, k] + cs[j] * H[j + 1, k]
                H[j, k] = t
            rho = float(np.hypot(H[k, k], H[k + 1, k]))
            if rho == 0.0 or not np.isfinite(rho):
                break
            cs[k], sn[k] = H[k, k] / rho, H[k + 1, k] / rho
            H[k, k], H[k + 1, k] = rho, 0.0
            g[k + 1] = -sn[k] * g[k]
            g[k] = cs[k] * g[k]
            its += 1
            k += 1
            hist.append(abs(g[k]) / bnorm)
            if hist[-1] <= rtol or hk[-1] == 0.0:
                break
            V[k].copy_(w)
            V[k].mul_(1.0 / float(hk[-1]))
        if k == 0:
            return its, hist
        y = np.linalg.solve(np.triu(H[:k, :k]), g[:k])
        if M is not None:
            w.zero_()
            maxpy(y, [V[j] for j in range(k)], w)
            M.solve(z, w)
            axpy(1.0, z, x)
        else:
            maxpy(y, [V[j] for j in range(k)], x)
        if hist[-1] <= rtol or its >= maxiter:
            return its, hist


GMRES_BASIS = {"f64": 0, "f32": 1}  # MI_BASIS_F64, MI_BASIS_F32
GMRES_CHECK_EVERY = 1  # the default of gmres_solver.solve / GMRES_dev: what tools/bench_gmres.py measured fastest (profiles/NOTES.md R12.1)


class gmres_solver:
    """mi_gmres_t: GMRES's definition above with a whole restart cycle enqueued on the device — the products, M, CGS2, the Givens
    rotations, the residual recurrence and the back-substitution — and one small read-back per check_every iterations instead of
    one stream drain per iteration (include/mi355_spmv.h, mi_gmres_*).  A: a bcsr4x4_matrix, a square csrmatrix or a
    dilu4 (the operator is then its apply_hat, M must be None, and the solve is in the hat variables: dilu4.gmres composes it);
    M: a bilu4 (the exact solve in the handle's current form), a bilu4.sweeps(..) view (either precision), a bilu4.exact("f32") view or None.  The solver owns its
    basis and work vectors; A and M must outlive it.  One solve at a time per solver, and per M.
    basis="f32" (MI_BASIS_F32, opt-in): the Krylov basis is stored in single precision, every projection is taken against the
    stored basis, and a converged recurrence is confirmed by the next cycle's true residual (basis_info()).
    Opt-in, with the bits of solve(): plan(b, x, ..) is the solve as graphs captured once and replayed; cycle() enqueues one whole
    restart cycle with no read-back, which the caller can capture into a graph of their own after prepare_stream(), and state()
    reads what it did."""

    def __init__(self, A, M=None, restart=30, basis="f64"):
        self._h = None
        if basis not in GMRES_BASIS:
            raise ValueError(f"basis: expected 'f64' or 'f32', got {basis!r}")
        self.basis = basis
        self.A, self.M = A, M
        self.n = 4 * A.nrows if isinstance(A, bcsr4x4_matrix) else 4 * A.nbrows if isinstance(A, dilu4) else A.n
        self.restart = int(restart)
        h = _vp()
        check(lib().mi_gmres_create_ex(self.n, self.restart, GMRES_BASIS[basis], _c.byref(h)))
        self._h = h
        if isinstance(A, bcsr4x4_matrix):
            check(lib().mi_gmres_set_operator_bcsr4(h, A.handle))
        elif isinstance(A, dilu4):  # the operator is A^ = apply_hat; M must be None (it is inside)
            if M is not None:
                raise ValueError("gmres_solver: a dilu4 operator takes no M (the preconditioner is inside apply_hat)")
            check(lib().mi_gmres_set_operator_dilu4(h, A.handle))
        else:
            check(lib().mi_gmres_set_operator_csr(h, A.handle))
        if M is not None:
            F, kind, fwd, bwd = M.gmres_args()
            # (the setter each kind has always gone through: the later kind has the later one)
            check((lib().mi_gmres_set_precond_ex if kind == GMRES_PC_EXACT_F32 else lib().mi_gmres_set_precond)(h, F, kind, fwd, bwd))

    @property
    def handle(self):
        if self._h is None:
            raise ValueError("gmres_solver: closed")
        return self._h

    def solve(self, b, x, rtol=1e-8, maxiter=300, check_every=GMRES_CHECK_EVERY):
        """(iterations, history, reason).  CUDA tensors: on torch's current stream, x (the initial guess, then the solution) is
        complete on that stream when the call returns; numpy arrays: copied in and out.  reason: 0 the initial guess met rtol,
        1 converged, 2 maxiter, 3 Krylov space exhausted, 4 a non-finite quantity or rho = 0."""
        its, reason = _c.c_int(), _c.c_int()
        hist = np.zeros(max(int(maxiter), 0) + 1)
        if _is_torch(b):
            check(lib().mi_gmres_solve_dev(self.handle, _dev_ptr(b, self.n, "b"), _dev_ptr(x, self.n, "x"), float(rtol), int(maxiter),
                                           int(check_every), _c.byref(its), _c.byref(reason), hist.ctypes.data, _stream_ptr()))
        else:
            xx = _host_f64(x, self.n, "x", writable=True)
            check(lib().mi_gmres_solve(self.handle, _host_f64(b, self.n, "b").ctypes.data, xx.ctypes.data, float(rtol), int(maxiter),
                                       int(check_every), _c.byref(its), _c.byref(reason), hist.ctypes.data))
        return its.value, [float(v) for v in hist[: its.value + 1]], reason.value

    def fetch_cycle(self):
        """(k, hraw, y, beta) of the last cycle of the last solve (mi_gmres_fetch_cycle): hraw (restart, restart + 2), row c the raw
        Gram-Schmidt column of step c with its norm at c + 1 (BuildKrylovBasis's layout); y (k,) the least-squares solution."""
        m = self.restart
        k, beta = _c.c_int(), _c.c_double()
        hraw, y = np.zeros((m, m + 2)), np.zeros(m)
        check(lib().mi_gmres_fetch_cycle(self.handle, _c.byref(k), hraw.ctypes.data, y.ctypes.data, _c.byref(beta)))
        return k.value, hraw, y[: k.value], beta.value

    def info(self):
        """dict(restart, device_bytes, readbacks_last, launches_last, wasted_steps_last) — mi_gmres_info."""
        m, rb, la, wa = (_c.c_int() for _ in range(4))
        by = _c.c_longlong()
        check(lib().mi_gmres_info(self.handle, _c.byref(m), _c.byref(by), _c.byref(rb), _c.byref(la), _c.byref(wa)))
        return dict(restart=m.value, device_bytes=by.value, readbacks_last=rb.value, launches_last=la.value, wasted_steps_last=wa.value)

    def basis_info(self):
        """dict(basis, basis_bytes, refused_last) — mi_gmres_basis_info: "f64" or "f32", the bytes of the stored basis, and the
        claims of the last solve's recurrence that the next cycle's true residual did not confirm (always 0 for "f64")."""
        kind, refused = _c.c_int(), _c.c_int()
        by = _c.c_longlong()
        check(lib().mi_gmres_basis_info(self.handle, _c.byref(kind), _c.byref(by), _c.byref(refused)))
        return dict(basis="f32" if kind.value == GMRES_BASIS["f32"] else "f64", basis_bytes=by.value, refused_last=refused.value)

    def prepare_stream(self):
        """Allocate, outside capture, whatever a first use on torch's current stream would allocate (mi_gmres_prepare_stream): call
        it on the stream a cycle() is going to be captured on."""
        check(lib().mi_gmres_prepare_stream(self.handle, _stream_ptr()))

    def cycle(self, b, x, first, rtol=1e-8, maxiter=300):
        """ONE whole restart cycle on torch's current stream with no read-back (mi_gmres_cycle_dev): capturable once the stream is
        prepared.  first: the start of a solve.  state() tells what it did."""
        check(lib().mi_gmres_cycle_dev(self.handle, _dev_ptr(b, self.n, "b"), _dev_ptr(x, self.n, "x"), 1 if first else 0, float(rtol),
                                       int(maxiter), _stream_ptr()))

    def state(self):
        """dict(its, k, done, reason, last, beta, history) of the record behind torch's current stream (mi_gmres_state; waits):
        history holds the entries of the cycle's k counted steps."""
        its, k, done, reason = (_c.c_int() for _ in range(4))
        last, beta = _c.c_double(), _c.c_double()
        hist = np.zeros(self.restart)
        check(lib().mi_gmres_state(self.handle, _stream_ptr(), _c.byref(its), _c.byref(k), _c.byref(done), _c.byref(reason), _c.byref(last),
                                   _c.byref(beta), hist.ctypes.data))
        return dict(its=its.value, k=k.value, done=bool(done.value), reason=reason.value, last=last.value, beta=beta.value,
                    history=[float(v) for v in hist[: k.value]])

    def plan(self, b, x, rtol=1e-8, maxiter=300, segment=None):
        """A gmres_plan: solve(b, x, rtol, maxiter) as replayed graphs of `segment` steps each (default: restart, one graph of
        steps per cycle).  b and x are baked in: refill them in place between solves."""
        return gmres_plan(self, b, x, rtol, maxiter, self.restart if segment is None else segment)

    def close(self):
        if self._h is not None:
            lib().mi_gmres_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class gmres_plan:
    """mi_gmres_plan_t (gmres_solver.plan): the solve of b, x (CUDA tensors, baked in: refill them in place) as graphs captured once
    and replayed, `segment` steps per graph; bit for bit gmres_solver.solve with the same arguments.  Stale (MiError, status 6)
    once the solver's operator or preconditioner is set again.  The solver, b and x must outlive it."""

    def __init__(self, S, b, x, rtol, maxiter, segment):
        self._h = None
        self.S, self.b, self.x, self.maxiter = S, b, x, int(maxiter)
        h = _vp()
        check(lib().mi_gmres_plan_create(S.handle, _dev_ptr(b, S.n, "b"), _dev_ptr(x, S.n, "x"), float(rtol), self.maxiter, int(segment),
                                         _c.byref(h)))
        self._h = h

    @property
    def handle(self):
        if self._h is None:
            raise ValueError("gmres_plan: closed")
        return self._h

    def solve(self):
        """(iterations, history, reason) on torch's current stream; x is complete on that stream when the call returns."""
        its, reason = _c.c_int(), _c.c_int()
        hist = np.zeros(max(self.maxiter, 0) + 1)
        check(lib().mi_gmres_plan_solve(self.handle, _c.byref(its), _c.byref(reason), hist.ctypes.data, _stream_ptr()))
        return its.value, [float(v) for v in hist[: its.value + 1]], reason.value

    def info(self):
        """dict(graphs, segment, replays_last, readbacks_last, wasted_steps_last) — mi_gmres_plan_info."""
        g, sg, rp, rb, wa = (_c.c_int() for _ in range(5))
        check(lib().mi_gmres_plan_info(self.handle, _c.byref(g), _c.byref(sg), _c.byref(rp), _c.byref(rb), _c.byref(wa)))
        return dict(graphs=g.value, segment=sg.value, replays_last=rp.value, readbacks_last=rb.value, wasted_steps_last=wa.value)

    def close(self):
        if self._h is not None:
            lib().mi_gmres_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def GMRES_dev(A, b, x, M=None, restart=30, rtol=1e-8, maxiter=300, check_every=GMRES_CHECK_EVERY, basis="f64"):
    """GMRES(A, b, x, M, restart, rtol, maxiter) through a gmres_solver made for the call: (iterations, history)."""
    S = gmres_solver(A, M, restart, basis)
    try:
        its, hist, _ = S.solve(b, x, rtol, maxiter, check_every)
    finally:
        S.close()
    return its, hist


# ------------------------------------------------------------------- BLAS-1

def _scalar_dev():
    import torch

    return torch.empty(1, dtype=torch.float64, device="cuda")


def dot(x, y):
    """sum x_i y_i (std::inner_product at mpk/SpMVmulti.cpp:147).  Device tensors: returns a 1-element device tensor."""
    n = int(x.numel() if _is_torch(x) else np.size(x))
    if _is_torch(x):
        out = _scalar_dev()
        check(lib().mi_dot_dev(n, _dev_ptr(x), _dev_ptr(y, n), _dev_ptr(out), _stream_ptr()))
        return out
    out = _c.c_double(0)
    check(lib().mi_dot(n, _host_f64(x).ctypes.data, _host_f64(y, n).ctypes.data, _c.byref(out)))
    return out.value


def axpy(a, x, y):
    """y += a x, in place."""
    n = int(x.numel() if _is_torch(x) else np.size(x))
    if _is_torch(x):
        check(lib().mi_axpy_dev(n, float(a), _dev_ptr(x), _dev_ptr(y, n), _stream_ptr()))
    else:
        yy = _host_f64(y, n, "y", writable=True)
        check(lib().mi_axpy(n, float(a), _host_f64(x).ctypes.data, yy.ctypes.data))
    return y


def orthogonalize(nrow, b, x1, x3, alpha=1e-8):
    """x3 = x1 - alpha*(b.x1)*b — orthogonalize(nrow, b, x1, x3, alpha), mpk/SpMVmulti.cpp:146-151.
    Returns beta = b.x1 (float for numpy inputs, 1-element device tensor otherwise)."""
    if _is_torch(b):
        beta = _scalar_dev()
        check(lib().mi_orthogonalize_dev(nrow, _dev_ptr(b, nrow), _dev_ptr(x1, nrow), _dev_ptr(x3, nrow), float(alpha),
                                         _dev_ptr(beta), _stream_ptr()))
        return beta
    out = _c.c_double(0)
    x3h = _host_f64(x3, nrow, "x3", writable=True)
    check(lib().mi_orthogonalize(nrow, _host_f64(b, nrow).ctypes.data, _host_f64(x1, nrow).ctypes.data,
                                 x3h.ctypes.data, float(alpha), _c.byref(out)))
    return out.value


def SpMV_CSR_dot(y, x, A, b):
    """y = A x and beta = b . y in one pass (mi_spmv_dot_dev): returns beta as a 1-element device tensor."""
    beta = _scalar_dev()
    check(lib().mi_spmv_dot_dev(A.handle, _dev_ptr(x, A.ncols, "x"), _dev_ptr(y, A.n, "y"), _dev_ptr(b, A.n, "b"), _dev_ptr(beta), _stream_ptr()))
    return beta


def SpMV_CSR_orthogonalize(x1, x, A, b, x3, alpha=1e-8):
    """SpMV_CSR(x1, x, A); orthogonalize(n, b, x1, x3, alpha) — mpk/SpMVmulti.cpp:563-565 — as two launches: the dot rides in
    the product's epilogue (mi_spmv_orthogonalize_dev).  Returns beta (1-element device tensor)."""
    beta = _scalar_dev()
    check(lib().mi_spmv_orthogonalize_dev(A.handle, _dev_ptr(x, A.ncols, "x"), _dev_ptr(x1, A.n, "x1"), _dev_ptr(b, A.n, "b"),
                                          _dev_ptr(x3, A.n, "x3"), float(alpha), _dev_ptr(beta), _stream_ptr()))
    return beta


def orthonormalize_against_basis(basis, y):
    """orthonormalize_against_basis(nrow, basis, y), mpk/2SpMV.cpp:13-28: for each basis vector in turn
    y -= (y . v) v on the y updated so far (nothing is normalised, like the reference).  y is updated in
    place; returns the m coefficients (numpy array, or a device tensor for device inputs).
    basis: sequence of m vectors (numpy rows or CUDA tensors)."""
    m = len(basis)
    if _is_torch(y):
        import torch
        n = int(y.numel())
        dots = torch.empty(max(m, 1), dtype=torch.float64, device=y.device)
        ptrs = (_vp * max(m, 1))(*[_dev_ptr(b, n, f"basis[{j}]").value for j, b in enumerate(basis)])
        check(lib().mi_orthonormalize_against_basis_dev(n, m, ptrs, _dev_ptr(y), _dev_ptr(dots), _stream_ptr()))
        return dots[:m]
    yy = _host_f64(y, None, "y", writable=True)
    n = yy.size
    rows = [_host_f64(b, n, f"basis[{j}]") for j, b in enumerate(basis)]
    ptrs = (_vp * max(m, 1))(*[r.ctypes.data for r in rows])
    dots = np.zeros(m)
    check(lib().mi_orthonormalize_against_basis(n, m, ptrs, yy.ctypes.data, dots.ctypes.data if m else None))
    return dots


def _dev_basis(basis, n, dtype=None):
    return (_vp * max(len(basis), 1))(*[_dev_ptr(b, n, f"basis[{j}]", dtype).value for j, b in enumerate(basis)])


def _basis_f32(basis):
    """A basis of torch.float32 CUDA vectors (the stored basis of a basis="f32" solver): the mi_*_f32_dev forms, y staying float64."""
    import torch
    return len(basis) > 0 and _is_torch(basis[0]) and basis[0].dtype == torch.float32


def round_f32(x, div=None):
    """(x32, x64) of mi_round_f32_dev: x32 = round32(x / div) as a float32 tensor — the division in float64 by the device scalar
    div (a 1-element CUDA tensor; None: no division), then rounded to nearest even, subnormals kept — and x64 = x32 widened to
    float64, in one pass.  x: a float64 CUDA tensor, left as it is."""
    import torch
    n = int(x.numel())
    x32 = torch.empty(n, dtype=torch.float32, device=x.device)
    x64 = torch.empty(n, dtype=torch.float64, device=x.device)
    check(lib().mi_round_f32_dev(n, _dev_ptr(x), _dev_ptr(div, 1, "div") if div is not None else None, _dev_ptr(x32, n, "x32", torch.float32),
                                 _dev_ptr(x64), _stream_ptr()))
    return x32, x64


def _host_basis(basis, n):
    rows = [_host_f64(b, n, f"basis[{j}]") for j, b in enumerate(basis)]
    return rows, (_vp * max(len(rows), 1))(*[r.ctypes.data for r in rows])  # rows: keeps converted copies alive


def mdot(basis, y):
    """VecMDot (src/solve_newton.c:1265): dots[j] = y . basis[j] in one pass over y per tile of vectors (mi_mdot*); every
    entry has the bits of dot(y, basis[j]).  Returns the m dots (numpy array, or a device tensor for device inputs)."""
    m = len(basis)
    if _is_torch(y):
        import torch
        n = int(y.numel())
        dots = torch.empty(max(m, 1), dtype=torch.float64, device=y.device)
        if _basis_f32(basis):
            check(lib().mi_mdot_f32_dev(n, m, _dev_basis(basis, n, torch.float32), _dev_ptr(y), _dev_ptr(dots), _stream_ptr()))
        else:
            check(lib().mi_mdot_dev(n, m, _dev_basis(basis, n), _dev_ptr(y), _dev_ptr(dots), _stream_ptr()))
        return dots[:m]
    yy = _host_f64(y)
    n = yy.size
    rows, ptrs = _host_basis(basis, n)
    dots = np.zeros(m)
    check(lib().mi_mdot(n, m, ptrs, yy.ctypes.data, dots.ctypes.data if m else None))
    return dots


def maxpy(coef, basis, y, negate=False, norm=False):
    """VecMAXPY (src/solve_newton.c:1265): y += sum_j a_j basis[j] in place, a_j = -coef[j] when negate else coef[j], as the
    per-element fma chain of m successive axpy (mi_maxpy*).  Device form: coef is a CUDA tensor (anything else is copied to
    one).  Returns y, or (y, ||y_new||_2) with norm=True — on the device the norm is accumulated while y is written
    (mi_maxpy_dev's d_norm_out) and has the bits of norm2(y)."""
    m = len(basis)
    if _is_torch(y):
        import torch
        n = int(y.numel())
        if not _is_torch(coef):
            coef = torch.as_tensor(np.asarray(coef, dtype=np.float64), device=y.device)
        out = _scalar_dev() if norm else None
        f32 = _basis_f32(basis)
        call = lib().mi_maxpy_f32_dev if f32 else lib().mi_maxpy_dev
        check(call(n, m, _dev_ptr(coef, m, "coef") if m else None, 1 if negate else 0, _dev_basis(basis, n, torch.float32 if f32 else None),
                   _dev_ptr(y), _dev_ptr(out) if norm else None, _stream_ptr()))
        return (y, out) if norm else y
    yy = _host_f64(y, None, "y", writable=True)
    n = yy.size
    rows, ptrs = _host_basis(basis, n)
    cc = _host_f64(coef, m, "coef")
    check(lib().mi_maxpy(n, m, cc.ctypes.data if m else None, 1 if negate else 0, ptrs, yy.ctypes.data))
    return (y, norm2(yy)) if norm else y


def maxpy_upto(count, coef, basis, y, negate=False):
    """maxpy(coef[:c], basis[:c], y, negate) with c = count[0] clamped to [0, len(basis)] and count an int32 CUDA tensor that the
    KERNELS read (mi_maxpy_upto*_dev): the call can be captured into a graph and replayed with another count.  The same bits as
    maxpy at that count; vectors and coefficients from c on are never loaded, and c = 0 leaves y as it is.  A float32 basis takes
    the float form.  Device tensors only.  Returns y."""
    import torch
    m = len(basis)
    if not (_is_torch(y) and _is_torch(count) and _is_torch(coef)):
        raise TypeError("maxpy_upto: count, coef and y must be CUDA tensors (there is no host form)")
    n = int(y.numel())
    f32 = _basis_f32(basis)
    call = lib().mi_maxpy_upto_f32_dev if f32 else lib().mi_maxpy_upto_dev
    check(call(n, m, _dev_ptr(count, 1, "count", torch.int32), _dev_ptr(coef, m, "coef") if m else None, 1 if negate else 0,
               _dev_basis(basis, n, torch.float32 if f32 else None), _dev_ptr(y), _stream_ptr()))
    return y


def cgs(basis, y, passes=2):
    """Classical Gram-Schmidt of y against basis, in place (mi_cgs_dev): per pass d = mdot(basis, y), y = maxpy(d, basis, y,
    negate=True); passes=2 is CGS2, what keeps a Krylov basis orthonormal.  Returns (h, norm): h the
    coefficients (pass 1, plus pass 2 with one rounded add) and norm = ||y_new||_2 — device tensors for device inputs,
    else a numpy array and a float (the host form composes the host calls: the same bits)."""
    m = len(basis)
    if passes not in (1, 2):
        raise ValueError(f"passes: expected 1 or 2, got {passes!r}")
    if _is_torch(y):
        import torch
        n = int(y.numel())
        h = torch.empty(max(m, 1), dtype=torch.float64, device=y.device)
        nrm = _scalar_dev()
        f32 = _basis_f32(basis)
        call = lib().mi_cgs_f32_dev if f32 else lib().mi_cgs_dev
        check(call(n, m, _dev_basis(basis, n, torch.float32 if f32 else None), _dev_ptr(y), passes, _dev_ptr(h), _dev_ptr(nrm), _stream_ptr()))
        return h[:m], nrm
    h = mdot(basis, y)
    maxpy(h, basis, y, negate=True)
    if passes == 2:
        d2 = mdot(basis, y)
        maxpy(d2, basis, y, negate=True)
        h = h + d2
    return h, norm2(y)


def norm2(x):
    """sqrt(sum x^2) — norm2, mpk/utils.cpp:131-136."""
    n = int(x.numel() if _is_torch(x) else np.size(x))
    if _is_torch(x):
        out = _scalar_dev()
        check(lib().mi_norm2_dev(n, _dev_ptr(x), _dev_ptr(out), _stream_ptr()))
        return out
    out = _c.c_double(0)
    check(lib().mi_norm2(n, _host_f64(x).ctypes.data, _c.byref(out)))
    return out.value


def rel_error(ref, test):
    """||ref - test||_2 / ||ref||_2 — rel_error, mpk/utils.cpp:138-143 (the parity metric)."""
    n = int(ref.numel() if _is_torch(ref) else np.size(ref))
    if _is_torch(ref):
        out = _scalar_dev()
        check(lib().mi_rel_error_dev(n, _dev_ptr(ref), _dev_ptr(test, n), _dev_ptr(out), _stream_ptr()))
        return out
    out = _c.c_double(0)
    check(lib().mi_rel_error(n, _host_f64(ref).ctypes.data, _host_f64(test, n).ctypes.data, _c.byref(out)))
    return out.value


def stream_read_us(nbytes, launches=20):
    """Microseconds per launch of a plain read sweep over nbytes of device memory (mi_stream_read_probe): this box's HBM rate."""
    us = _c.c_double()
    check(lib().mi_stream_read_probe(int(nbytes), int(launches), _c.byref(us)))
    return us.value


def flush_cache(sync=True):
    """mpk/utils.cpp:146-154 evicts the CPU caches before a timed call.  The GPU analogue evicts the L2s and the 256 MiB
    Infinity Cache (512 MiB device fill + 512 MiB read sweep).  sync=False: enqueued on the current stream without the
    closing synchronise, so that the next launch starts on cold caches but not on an idle GPU (mi_flush_cache_async)."""
    if sync:
        check(lib().mi_flush_cache())
    else:
        check(lib().mi_flush_cache_async(_stream_ptr()))
