"""ctypes mirror of include/mg3d.h plus a `Solver` class that follows the reference's Solver* facade
(mg_3d.h:107-144, 275-293, 1412-1467).  No compute happens here; every call goes into libmg3d.so and
raises `Mg3dError` when the library (or a GPU) is missing -- there is no CPU fallback."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
dp = C.POINTER(C.c_double)
fp = C.POINTER(C.c_float)

MG3D_U, MG3D_D, MG3D_R = 0, 1, 2
MG3D_PERIODIC_I, MG3D_PERIODIC_J, MG3D_PERIODIC_K = 1, 2, 4
STAGES = 7
# mg3d_ctx_sweep_taken: MG3D_SWEEP_KIND_* and the MG3D_SWEEP_TAKEN_* fields in order
SWEEP_KINDS = {"passes": 0, "passes_res": 1, "tap": 2, "leg_down": 3, "leg_up": 4}
SWEEP_TAKEN_FIELDS = ("S", "RES", "RJ", "NW", "PF", "ND", "DZ", "CI", "blocks", "xcd_remap", "ntj", "ntk", "PRO", "RST", "DP",
                      "TAP", "N")
_ERR = {1: "bad argument", 2: "no device", 3: "HIP error", 4: "allocation failed", 5: "bad state"}


class Mg3dError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"mg3d error {code} ({_ERR.get(code, '?')}): {msg}")
        self.code = code


def lib_path():
    # MG3D_LIB_PATH: an alternative build of the same library (A/B measurements of kernel variants on one box)
    return os.environ.get("MG3D_LIB_PATH") or os.path.join(_HERE, "lib", "libmg3d.so")


_lib = None

MG3D_F64, MG3D_F32, MG3D_U8 = 0, 1, 2  # mg3d_array.dtype (MG3D_U8: mg3d_ctx_set_mask_device only)
MG3D_I32 = 3  # mg3d_vec.dtype of the fate vector of mg3d_particle_push_device and of the vectors of the reorder
MG3D_PERMUTE_MAX_VECS = 16  # vectors per launch of mg3d_particle_permute_device
# the fates of mg3d_particle_push: 0 alive, 1..255 the label of the conductor that absorbed the particle, MG3D_FATE_FACE + f
# for face f = 0..5 (ilo, ihi, jlo, jhi, klo, khi), MG3D_FATE_INVALID; MG3D_FATE_SLOTS counters (mg3d_particle_counts)
MG3D_FATE_ALIVE, MG3D_FATE_FACE, MG3D_FATE_INVALID, MG3D_FATE_SLOTS = 0, 256, 262, 263


class mg3d_array(C.Structure):
    """mg3d_array: a dense-indexed N x N x N array in device memory -- element (i, j, k) is
    ptr[stride[0]*i + stride[1]*j + stride[2]*k], strides in elements.  array_desc() builds one from a torch tensor."""
    _fields_ = [("ptr", C.c_void_p), ("dtype", C.c_int), ("stride", C.c_longlong * 3)]


_ap = C.POINTER(mg3d_array)


class mg3d_vec(C.Structure):
    """mg3d_vec: a 1-D strided vector in device memory -- element m is ptr[stride*m], stride in elements.  vec_desc()
    builds one from a 1-D torch tensor."""
    _fields_ = [("ptr", C.c_void_p), ("dtype", C.c_int), ("stride", C.c_longlong)]


_vp = C.POINTER(mg3d_vec)


class mg3d_push_params(C.Structure):
    """mg3d_push_params: the step dt, the scale of the force field (scale * grad u), a constant acceleration, the drag."""
    _fields_ = [("dt", C.c_double), ("scale", C.c_double), ("accel", C.c_double * 3), ("drag", C.c_double)]


# name -> (restype, argtypes); this table is also what tests/test_abi.py checks against include/mg3d.h
SIGNATURES = {
    "mg3d_last_error": (C.c_char_p, []),
    "mg3d_stage_name": (C.c_char_p, [C.c_int]),
    "mg3d_device_count": (C.c_int, []),
    "mg3d_ctx_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_void_p)]),
    "mg3d_ctx_destroy": (C.c_int, [C.c_void_p]),
    "mg3d_ctx_num_levels": (C.c_int, [C.c_void_p]),
    "mg3d_ctx_level_n": (C.c_int, [C.c_void_p, C.c_int]),
    "mg3d_ctx_level_h": (C.c_double, [C.c_void_p, C.c_int]),
    "mg3d_ctx_set_smooth_iters": (C.c_int, [C.c_void_p, C.c_int]),
    "mg3d_ctx_set_keep_residual": (C.c_int, [C.c_void_p, C.c_int]),
    "mg3d_ctx_build_coarse": (C.c_int, [C.c_void_p, C.c_double]),
    "mg3d_ctx_set_lu": (C.c_int, [C.c_void_p, dp]),
    "mg3d_ctx_set_shift": (C.c_int, [C.c_void_p, C.c_double]),
    "mg3d_ctx_get_shift": (C.c_int, [C.c_void_p, dp]),
    "mg3d_ctx_set_coefficient": (C.c_int, [C.c_void_p, dp]),
    "mg3d_ctx_has_coefficient": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "mg3d_ctx_get_coefficient": (C.c_int, [C.c_void_p, C.c_int, dp]),
    "mg3d_ctx_set_periodic": (C.c_int, [C.c_void_p, C.c_int]),
    "mg3d_ctx_get_periodic": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "mg3d_ctx_set_neumann": (C.c_int, [C.c_void_p, C.c_int]),
    "mg3d_ctx_get_neumann": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "mg3d_upload": (C.c_int, [C.c_void_p, C.c_int, C.c_int, dp]),
    "mg3d_download": (C.c_int, [C.c_void_p, C.c_int, C.c_int, dp]),
    "mg3d_zero": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "mg3d_sync": (C.c_int, [C.c_void_p]),
    "mg3d_device_view": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int),
                                   C.POINTER(C.c_long)]),
    "mg3d_upload_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _ap, C.c_void_p]),
    "mg3d_download_device": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _ap, C.c_void_p]),
    "mg3d_step_set_source_device": (C.c_int, [C.c_void_p, _ap, C.c_void_p]),
    "mg3d_ctx_set_coefficient_device": (C.c_int, [C.c_void_p, _ap, C.c_void_p]),
    "mg3d_ctx_set_shift_field": (C.c_int, [C.c_void_p, dp]),
    "mg3d_ctx_set_shift_field_device": (C.c_int, [C.c_void_p, _ap, C.c_void_p]),
    "mg3d_ctx_has_shift_field": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "mg3d_ctx_get_shift_field": (C.c_int, [C.c_void_p, C.c_int, dp]),
    "mg3d_ctx_set_mask": (C.c_int, [C.c_void_p, C.POINTER(C.c_ubyte)]),
    "mg3d_ctx_set_mask_device": (C.c_int, [C.c_void_p, _ap, C.c_void_p]),
    "mg3d_ctx_has_mask": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "mg3d_ctx_get_mask": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_ubyte)]),
    "mg3d_ctx_set_mask_coarsening": (C.c_int, [C.c_void_p, C.c_int]),
    "mg3d_ctx_get_mask_coarsening": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "mg3d_smooth": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "mg3d_residual": (C.c_int, [C.c_void_p, C.c_int, C.c_int, dp]),
    "mg3d_smooth_residual": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, dp]),
    "mg3d_smooth_restrict": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "mg3d_restrict": (C.c_int, [C.c_void_p, C.c_int]),
    "mg3d_prolong": (C.c_int, [C.c_void_p, C.c_int]),
    "mg3d_coarse_solve": (C.c_int, [C.c_void_p]),
    "mg3d_l2norm": (C.c_int, [C.c_void_p, C.c_int, C.c_int, dp]),
    "mg3d_vcycle": (C.c_int, [C.c_void_p, C.c_int, dp]),
    "mg3d_vcycles": (C.c_int, [C.c_void_p, C.c_int, dp]),
    "mg3d_pcg_solve": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_int, dp, C.c_void_p]),
    "mg3d_wpcg_solve": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_int, dp, C.c_void_p]),
    "mg3d_fmg_initialize": (C.c_int, [C.c_void_p]),
    "mg3d_fmg_interpolate": (C.c_int, [C.c_void_p, C.c_int]),
    "mg3d_fmg_solve": (C.c_int, [C.c_void_p, C.c_int, dp]),
    "mg3d_step_setup": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double]),
    "mg3d_step_set_source": (C.c_int, [C.c_void_p, dp]),
    "mg3d_step_advance": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, dp, C.c_void_p]),
    "mg3d_nl_setup": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double]),
    "mg3d_nl_set_weight": (C.c_int, [C.c_void_p, dp]),
    "mg3d_nl_set_weight_device": (C.c_int, [C.c_void_p, _ap, C.c_void_p]),
    "mg3d_nl_residual": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double)]),
    "mg3d_nl_solve": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, dp,
                                C.c_void_p]),
    "mg3d_field_gradient": (C.c_int, [C.c_void_p, C.c_double, dp, dp, dp]),
    "mg3d_field_gradient_device": (C.c_int, [C.c_void_p, C.c_double, C.POINTER(_ap), C.c_void_p]),
    "mg3d_field_flux": (C.c_int, [C.c_void_p, C.c_int, dp]),
    "mg3d_field_energy": (C.c_int, [C.c_void_p, dp]),
    "mg3d_field_sample": (C.c_int, [C.c_void_p, C.c_longlong, dp, C.c_double, dp, dp]),
    "mg3d_field_sample_device": (C.c_int, [C.c_void_p, C.c_longlong, C.POINTER(_vp), C.c_double, _vp, C.POINTER(_vp),
                                           C.c_void_p]),
    "mg3d_deposit": (C.c_int, [C.c_void_p, C.c_longlong, dp, dp, C.c_double]),
    "mg3d_deposit_device": (C.c_int, [C.c_void_p, C.c_longlong, C.POINTER(_vp), _vp, C.c_double, C.c_void_p]),
    "mg3d_particle_push_device": (C.c_int, [C.c_void_p, C.c_longlong, C.POINTER(_vp), C.POINTER(_vp), _vp, _vp,
                                            C.POINTER(mg3d_push_params), C.c_void_p]),
    "mg3d_particle_push": (C.c_int, [C.c_void_p, C.c_longlong, dp, dp, dp, C.POINTER(C.c_int),
                                     C.POINTER(mg3d_push_params)]),
    "mg3d_particle_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong), C.c_int]),
    "mg3d_particle_sort_device": (C.c_int, [C.c_void_p, C.c_longlong, C.POINTER(_vp), _vp, C.c_int, _vp, C.c_void_p,
                                            C.c_void_p]),
    "mg3d_particle_permute_device": (C.c_int, [C.c_void_p, C.c_longlong, _vp, C.c_int, C.POINTER(_vp), C.POINTER(_vp),
                                               C.c_void_p]),
    "mg3d_particle_sort": (C.c_int, [C.c_void_p, C.c_longlong, dp, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int),
                                     C.POINTER(C.c_longlong)]),
    "mg3d_fill_boundary": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "mg3d_timing_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "mg3d_timing_reset": (C.c_int, [C.c_void_p]),
    "mg3d_timing_get": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), dp]),
    "mg3d_kernel_name": (C.c_char_p, [C.c_int]),
    "mg3d_kernel_time_get": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), dp]),
    "mg3d_comm_unique_id": (C.c_int, [C.c_void_p]),
    "mg3d_dist_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                   C.POINTER(C.c_void_p)]),
    "mg3d_dist_destroy": (C.c_int, [C.c_void_p]),
    "mg3d_dist_comm_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mg3d_dist_first_level": (C.c_int, [C.c_void_p]),
    "mg3d_dist_halo": (C.c_int, [C.c_void_p]),
    "mg3d_dist_carried_cycles": (C.c_int, [C.c_void_p]),
    "mg3d_dist_legs_cycles": (C.c_int, [C.c_void_p]),
    "mg3d_dist_set_keep_residual": (C.c_int, [C.c_void_p, C.c_int]),
    "mg3d_dist_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "mg3d_ctx_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "mg3d_ctx_get_option": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_int)]),
    "mg3d_option_name": (C.c_char_p, [C.c_int]),
    "mg3d_ctx_dzero_planes": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mg3d_ctx_dnone_launches": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong)]),
    "mg3d_ctx_sweep_taken": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_ulonglong),
                                       C.POINTER(C.c_ulonglong)]),
    "mg3d32_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "mg3d32_timing_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "mg3d32_kernel_name": (C.c_char_p, [C.c_int]),
    "mg3d32_kernel_time_get": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), dp]),
    "mg3d_dist_build_coarse": (C.c_int, [C.c_void_p, C.c_double]),
    "mg3d_dist_set_shift": (C.c_int, [C.c_void_p, C.c_double]),
    "mg3d_dist_set_coefficient": (C.c_int, [C.c_void_p, dp]),
    "mg3d_dist_has_coefficient": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "mg3d_dist_get_coefficient": (C.c_int, [C.c_void_p, C.c_int, dp]),
    "mg3d_dist_upload": (C.c_int, [C.c_void_p, C.c_int, C.c_int, dp]),
    "mg3d_dist_download": (C.c_int, [C.c_void_p, C.c_int, C.c_int, dp]),
    "mg3d_dist_vcycles": (C.c_int, [C.c_void_p, C.c_int, dp]),
    "mg3d_dist_sync": (C.c_int, [C.c_void_p]),
    "mg3d_slab_halo": (C.c_int, [C.c_int]),
    "mg3d_slab_first_level": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "mg3d_slab_owned": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                                  C.POINTER(C.c_int)]),
    "mg3d_debug_tiny_stamps": (C.c_int, [C.POINTER(C.c_longlong)]),
    "mg3d_dist_plan": (C.c_int, [C.c_int] * 7 + [C.c_void_p, C.c_int]),
    "mg3d32_dist_plan": (C.c_int, [C.c_int] * 7 + [C.c_void_p, C.c_int]),
    "mg3d_dist_timing_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "mg3d_dist_timing_get": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "mg3d_host_smooth": (C.c_int, [dp, dp, C.c_int, C.c_double, C.c_int, C.c_int]),
    "mg3d_host_residual": (C.c_int, [dp, dp, C.c_int, C.c_double, dp, dp]),
    "mg3d_host_restrict": (C.c_int, [dp, C.c_int, dp, C.c_int]),
    "mg3d_host_prolong": (C.c_int, [dp, C.c_int, dp, C.c_int]),
    "mg3d_host_lu_solve": (C.c_int, [dp, C.c_int, dp, dp]),
    "mg3d_host_vcycle": (C.c_int, [C.POINTER(dp), C.POINTER(dp), C.POINTER(dp), C.c_double, C.c_int, C.c_int, C.c_int,
                                   C.c_int, dp, dp, C.POINTER(C.c_int), dp]),
    "mg3d_bc_func": (C.c_double, [C.c_double, C.c_double, C.c_double]),
    "mg3d_fill_boundary_host": (None, [dp, C.c_int, C.c_double]),
    "mg3d_coarse_matrix": (None, [dp, C.c_int, C.c_double]),
    "mg3d_coarse_matrix_shift": (None, [dp, C.c_int, C.c_double, C.c_double]),
    "mg3d_coarse_matrix_coef": (None, [dp, C.c_int, C.c_double, dp, C.c_double]),
    "mg3d_coarse_matrix_periodic": (None, [dp, C.c_int, C.c_double, dp, C.c_double, C.c_int]),
    "mg3d_coarse_matrix_bc": (None, [dp, C.c_int, C.c_double, dp, C.c_double, C.c_int, C.c_int]),
    "mg3d_coarse_matrix_mask": (None, [dp, C.c_int, C.c_double, dp, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_ubyte)]),
    "mg3d_coarse_matrix_field": (None, [dp, C.c_int, C.c_double, dp, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_ubyte), dp]),
    "mg3d_neumann_fold_flux": (C.c_int, [dp, dp, C.c_int, C.c_double, C.c_int, C.POINTER(dp)]),
    "mg3d_lu_factor": (None, [dp, C.c_int]),
    "mg3d_l2norm_host": (C.c_double, [dp, C.c_long]),
    "mg3d_smooth_edges_host": (None, [dp, C.c_int]),
    "mg3d_write_vtk": (C.c_int, [C.c_char_p, dp, C.c_double, C.c_int]),
    "mg3d_host_alloc": (C.c_int, [C.c_size_t, C.POINTER(C.c_void_p)]),
    "mg3d_host_free": (C.c_int, [C.c_void_p]),
    # single precision / damped Jacobi / F-cycle variant (parity unpinned)
    "mg3d32_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_void_p)]),
    "mg3d32_destroy": (C.c_int, [C.c_void_p]),
    "mg3d32_level_n": (C.c_int, [C.c_void_p, C.c_int]),
    "mg3d32_upload": (C.c_int, [C.c_void_p, C.c_int, C.c_int, fp]),
    "mg3d32_download": (C.c_int, [C.c_void_p, C.c_int, C.c_int, fp]),
    "mg3d32_zero": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "mg3d32_sync": (C.c_int, [C.c_void_p]),
    "mg3d32_fill_boundary": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "mg3d32_smooth": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "mg3d32_residual": (C.c_int, [C.c_void_p, C.c_int, C.c_int, dp]),
    "mg3d32_restrict": (C.c_int, [C.c_void_p, C.c_int]),
    "mg3d32_prolong": (C.c_int, [C.c_void_p, C.c_int]),
    "mg3d32_coarse_solve": (C.c_int, [C.c_void_p]),
    "mg3d32_vcycles": (C.c_int, [C.c_void_p, C.c_int, dp]),
    "mg3d32_fmg_initialize": (C.c_int, [C.c_void_p]),
    "mg3d_es_default_params": (C.c_int, [C.c_void_p]),
    "mg3d_es_coarse_matrix": (None, [dp, C.c_int, C.c_double, C.c_void_p]),
    "mg3d_es_setup": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mg3d_es_smooth": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "mg3d_es_vcycles": (C.c_int, [C.c_void_p, C.c_int, dp]),
    "mg3d32_slab_halo": (C.c_int, [C.c_int]),
    "mg3d32_dist_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_void_p,
                                     C.c_int, C.POINTER(C.c_void_p)]),
    "mg3d32_dist_destroy": (C.c_int, [C.c_void_p]),
    "mg3d32_dist_first_level": (C.c_int, [C.c_void_p]),
    "mg3d32_dist_halo": (C.c_int, [C.c_void_p]),
    "mg3d32_dist_comm_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mg3d32_dist_upload": (C.c_int, [C.c_void_p, C.c_int, C.c_int, fp]),
    "mg3d32_dist_download": (C.c_int, [C.c_void_p, C.c_int, C.c_int, fp]),
    "mg3d32_dist_zero": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "mg3d32_dist_fill_boundary": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "mg3d32_dist_vcycles": (C.c_int, [C.c_void_p, C.c_int, dp]),
    "mg3d32_dist_fmg_initialize": (C.c_int, [C.c_void_p]),
    "mg3d32_dist_sync": (C.c_int, [C.c_void_p]),
}


NEUMANN_FACES = ("ilo", "ihi", "jlo", "jhi", "klo", "khi")  # bit f of the MG3D_NEUMANN_* mask
MASK_COARSENING = {"inject": 0, "keep": 1}  # MG3D_MASK_INJECT, MG3D_MASK_KEEP


class PcgInfo(C.Structure):
    """mg3d_pcg_info: what mg3d_pcg_solve reports"""
    _fields_ = [("iterations", C.c_int), ("converged", C.c_int), ("r0_norm", C.c_double), ("r_norm", C.c_double)]


class WpcgInfo(C.Structure):
    """mg3d_wpcg_info: what mg3d_wpcg_solve reports"""
    _fields_ = [("iterations", C.c_int), ("converged", C.c_int), ("r0_norm", C.c_double), ("r_norm", C.c_double),
                ("singular", C.c_int), ("rhs_mean", C.c_double)]


class StepInfo(C.Structure):
    """mg3d_step_info: what mg3d_step_advance reports"""
    _fields_ = [("steps", C.c_int), ("iterations", C.c_int), ("converged", C.c_int), ("time", C.c_double)]


STEP_METHODS = {"vcycles": 0, "wpcg": 1}  # MG3D_STEP_VCYCLES, MG3D_STEP_WPCG


class NlInfo(C.Structure):
    """mg3d_nl_info: what mg3d_nl_solve reports"""
    _fields_ = [("iterations", C.c_int), ("converged", C.c_int), ("halvings", C.c_int), ("linear_iterations", C.c_int),
                ("last_lambda", C.c_double), ("norm0", C.c_double), ("norm", C.c_double)]


NL_KINDS = {"exp": 0, "sinh": 1}  # MG3D_NL_EXP, MG3D_NL_SINH


class EsParams(C.Structure):
    """mg3d_es_params: the mixed-boundary problem of mg_3d_bkup.c:12-18 (defaults = the reference's #defines)."""
    _fields_ = [("length", C.c_double), ("capillary_radius", C.c_double), ("extractor_inner_radius", C.c_double),
                ("extractor_outer_radius", C.c_double), ("capillary_voltage", C.c_double), ("extractor_voltage", C.c_double)]

    @staticmethod
    def default():
        p = EsParams()
        check(lib().mg3d_es_default_params(C.byref(p)))
        return p


def lib():
    """Load libmg3d.so (built in-tree by `make -C multigrid_parallel_amd/csrc`)."""
    global _lib
    if _lib is None:
        path = lib_path()
        if not os.path.exists(path):
            raise Mg3dError(2, f"{path} not built; run __graft_entry__.build() (there is no CPU fallback)")
        L = C.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name, None)
            if fn is None and os.environ.get("MG3D_LIB_PATH"):
                continue  # an older build used as an A/B reference may lack newer entry points
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def P(a):
    if a is None:
        return None
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"], "need contiguous float64"
    return a.ctypes.data_as(dp)


def check(rc):
    if rc != 0:
        raise Mg3dError(rc, lib().mg3d_last_error().decode(errors="replace"))


def array_desc(t, writable=False, shape=None):
    """The mg3d_array of a 3-D float64 / float32 torch tensor: data_ptr(), the dtype code and stride() in elements --
    any view is described as it is, nothing is copied.  TypeError for anything else; ValueError for a shape other than
    `shape` (when given) and, with writable=True, for a zero stride (an expanded tensor cannot be written).  The tensor
    must stay alive until the call that takes the descriptor has returned.  torch is imported here, not with the package."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"array_desc: need a torch.Tensor, got {type(t).__name__}")
    if t.dtype not in (torch.float64, torch.float32):
        raise TypeError(f"array_desc: need float64 or float32, got {t.dtype}")
    if t.dim() != 3:
        raise TypeError(f"array_desc: need a 3-D tensor, got {t.dim()} dimensions")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"array_desc: need shape {tuple(shape)}, got {tuple(t.shape)}")
    st = t.stride()
    if writable and any(v == 0 for v in st):
        raise ValueError(f"array_desc: a tensor that is written needs every stride >= 1, got {tuple(st)}")
    return mg3d_array(t.data_ptr(), MG3D_F64 if t.dtype == torch.float64 else MG3D_F32, (C.c_longlong * 3)(*st))


def _device_args(t, who, shape, writable=False):
    """descriptor and stream handle of a GPU tensor for the mg3d_*_device entry points"""
    import torch
    a = array_desc(t, writable=writable, shape=shape)
    if not t.is_cuda:
        raise ValueError(f"{who}: need a tensor on the GPU, got device {t.device}")
    return a, C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def vec_desc(t, writable=False, count=None, fate=False):
    """The mg3d_vec of a 1-D float64 / float32 torch tensor: data_ptr(), the dtype code and stride(0) in elements -- any
    view is described as it is, nothing is copied.  TypeError for anything else; ValueError for a length other than
    `count` (when given) and, with writable=True, for a zero stride.  fate=True: the fate vector of push_tensor, int32
    and nothing else (MG3D_I32), always written.  The tensor must stay alive until the call that takes the descriptor has
    returned."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"vec_desc: need a torch.Tensor, got {type(t).__name__}")
    if fate:
        if t.dtype != torch.int32:
            raise TypeError(f"vec_desc: a fate vector is int32, got {t.dtype}")
        writable = True
    elif t.dtype not in (torch.float64, torch.float32):
        raise TypeError(f"vec_desc: need float64 or float32, got {t.dtype}")
    if t.dim() != 1:
        raise TypeError(f"vec_desc: need a 1-D tensor, got {t.dim()} dimensions")
    if count is not None and t.shape[0] != count:
        raise ValueError(f"vec_desc: need {count} elements, got {t.shape[0]}")
    st = t.stride(0) if t.shape[0] > 1 else max(t.stride(0), 1)
    if writable and st == 0:
        raise ValueError("vec_desc: a tensor that is written needs a stride >= 1, got 0")
    if fate:
        return mg3d_vec(t.data_ptr(), MG3D_I32, st)
    return mg3d_vec(t.data_ptr(), MG3D_F64 if t.dtype == torch.float64 else MG3D_F32, st)


def _data_vec(t, who, writable=False, count=None):
    """The mg3d_vec of a 1-D float64 / float32 / int32 torch tensor, any view: the vectors of the reorder (sort_tensor,
    permute_tensors), which take MG3D_I32 beside the two float types."""
    import torch
    codes = {torch.float64: MG3D_F64, torch.float32: MG3D_F32, torch.int32: MG3D_I32}
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{who}: need a torch.Tensor, got {type(t).__name__}")
    if t.dtype not in codes:
        raise TypeError(f"{who}: need float64, float32 or int32, got {t.dtype}")
    if t.dim() != 1:
        raise TypeError(f"{who}: need a 1-D tensor, got {t.dim()} dimensions")
    if count is not None and t.shape[0] != count:
        raise ValueError(f"{who}: need {count} elements, got {t.shape[0]}")
    st = t.stride(0) if t.shape[0] > 1 else max(t.stride(0), 1)
    if writable and st == 0:
        raise ValueError(f"{who}: a tensor that is written needs a stride >= 1, got 0")
    return mg3d_vec(t.data_ptr(), codes[t.dtype], st)


def _vec_ptrs(descs):
    return (_vp * 3)(*[C.pointer(d) if d is not None else _vp() for d in descs])


def _position_args(pos, who, writable=False):
    """the three position vectors of an (M, 3) tensor (any view) or of a sequence of three 1-D tensors of one length, all on
    one GPU: (descriptors, M, device, stream handle)"""
    import torch
    if isinstance(pos, torch.Tensor):
        if pos.dim() != 2 or pos.shape[1] != 3:
            raise ValueError(f"{who}: positions need shape (M, 3), got {tuple(pos.shape)}")
        parts = [pos[:, 0], pos[:, 1], pos[:, 2]]
    else:
        parts = list(pos)
        if len(parts) != 3:
            raise ValueError(f"{who}: positions need three coordinate vectors, got {len(parts)}")
    for t in parts:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{who}: need torch tensors, got {type(t).__name__}")
        if not t.is_cuda:
            raise ValueError(f"{who}: need tensors on the GPU, got device {t.device}")
        if t.device != parts[0].device:
            raise ValueError(f"{who}: positions on different devices ({t.device}, {parts[0].device})")
    if any(t.dim() != 1 for t in parts):
        raise ValueError(f"{who}: each coordinate vector must be 1-D")
    M = parts[0].shape[0]
    descs = [vec_desc(t, writable=writable, count=M) for t in parts]
    return descs, M, parts[0].device, C.c_void_p(torch.cuda.current_stream(parts[0].device).cuda_stream)


class Solver:
    """Device-resident solver context.  Method names follow the reference facade:

    Solver(c, L, nu)                     ~ SolverInitialize(argv = c, L, nu)      mg_3d.h:107
    get_details()                        ~ SolverGetDetails (N, h; builds the LU)   mg_3d.h:275
    setup_boundary_conditions()          ~ SolverSetupBoundaryConditions            mg_3d.h:1412
    get_initial_residual()               ~ SolverGetInitialResidual                 mg_3d.h:1430
    lin_solve()                          ~ SolverLinSolve (one V-cycle, its norm)   mg_3d.h:1415
    get_residual()                       ~ SolverGetResidual                        mg_3d.h:1425
    finalize()                           ~ SolverFinalize                           mg_3d.h:1452
    """

    def __init__(self, coarse_pts, num_levels, smooth_iters, grid_length=1.0):
        self._h = C.c_void_p()
        self.L = lib()
        check(self.L.mg3d_ctx_create(coarse_pts, num_levels, smooth_iters, grid_length, C.byref(self._h)))
        self.c, self.num_levels, self.nu = coarse_pts, num_levels, smooth_iters
        self.N = self.L.mg3d_ctx_level_n(self._h, num_levels - 1)
        self.h = self.L.mg3d_ctx_level_h(self._h, num_levels - 1)

    # -- lifetime
    def finalize(self):
        if self._h:
            check(self.L.mg3d_ctx_destroy(self._h))
            self._h = C.c_void_p()

    close = finalize

    def __del__(self):
        try:
            self.finalize()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.finalize()

    def set_keep_residual(self, keep=True):
        check(self.L.mg3d_ctx_set_keep_residual(self._h, int(keep)))

    def set_option(self, key, value):
        """mg3d_ctx_set_option: launch / schedule policy by key (include/mg3d.h has the table)."""
        check(self.L.mg3d_ctx_set_option(self._h, key.encode(), int(value)))

    def get_option(self, key):
        v = C.c_int(0)
        check(self.L.mg3d_ctx_get_option(self._h, key.encode(), C.byref(v)))
        return v.value

    def options(self):
        out, i = {}, 0
        while self.L.mg3d_option_name(i):
            k = self.L.mg3d_option_name(i).decode()
            out[k] = self.get_option(k)
            i += 1
        return out

    def dzero_planes(self):
        """mg3d_ctx_dzero_planes: (planes of the finest level's d the zero map holds, state: 0 off, 1 to be scanned, 2 valid)."""
        n, st = C.c_int(0), C.c_int(0)
        check(self.L.mg3d_ctx_dzero_planes(self._h, C.byref(n), C.byref(st)))
        return n.value, st.value

    def dnone_launches(self):
        """mg3d_ctx_dnone_launches: launches that ran a kernel without d because the zero map was full."""
        n = C.c_ulonglong(0)
        check(self.L.mg3d_ctx_dnone_launches(self._h, C.byref(n)))
        return n.value

    def sweep_taken(self, kind):
        """mg3d_ctx_sweep_taken: the fused sweep launches of one kind (a key of SWEEP_KINDS) this context has taken, as
        (launches of the kind, the distinct records as dicts over SWEEP_TAKEN_FIELDS plus "count", most recent first)."""
        out, recs, which = (C.c_int * len(SWEEP_TAKEN_FIELDS))(), [], 0
        count, launches = C.c_ulonglong(0), C.c_ulonglong(0)
        while True:
            check(self.L.mg3d_ctx_sweep_taken(self._h, SWEEP_KINDS[kind], which, out, C.byref(count), C.byref(launches)))
            if count.value == 0:
                return launches.value, recs
            recs.append(dict(zip(SWEEP_TAKEN_FIELDS, out), count=count.value))
            which += 1

    # -- geometry
    def level_n(self, level):
        return self.L.mg3d_ctx_level_n(self._h, level)

    def level_h(self, level):
        return self.L.mg3d_ctx_level_h(self._h, level)

    # -- facade
    def get_details(self, coarse_h=None):
        """Builds + factors the coarsest operator with spacing h*2^(L-1) (mg_3d.h:287) unless given."""
        ch = self.h * (1 << (self.num_levels - 1)) if coarse_h is None else coarse_h
        check(self.L.mg3d_ctx_build_coarse(self._h, ch))
        return self.N, self.h

    def set_lu(self, LU):
        check(self.L.mg3d_ctx_set_lu(self._h, P(LU)))

    def set_shift(self, sigma):
        """mg3d_ctx_set_shift: solve the screened equation  Laplacian(u) - sigma*u = d  (sigma >= 0; 0 is Poisson).
        Rebuilds a coarse factor of get_details(); drops one given to set_lu."""
        check(self.L.mg3d_ctx_set_shift(self._h, float(sigma)))

    def get_shift(self):
        sigma = C.c_double(0.)
        check(self.L.mg3d_ctx_get_shift(self._h, C.byref(sigma)))
        return sigma.value

    def set_coefficient(self, eps):
        """mg3d_ctx_set_coefficient: solve  div(eps grad u) - sigma*u = d  with eps > 0 given at every point of the finest
        level ((N, N, N) or flat float64; coarser levels take it by injection).  None: the constant operator again.
        Rebuilds a coarse factor of get_details(); drops one given to set_lu."""
        if eps is None:
            check(self.L.mg3d_ctx_set_coefficient(self._h, None))
            return
        eps = np.asarray(eps)
        if eps.dtype != np.float64:
            raise TypeError(f"set_coefficient: need float64, got {eps.dtype}")
        if eps.size != self.N ** 3 or eps.shape not in ((self.N ** 3,), (self.N, self.N, self.N)):
            raise ValueError(f"set_coefficient: need shape ({self.N},)*3 or ({self.N ** 3},), got {eps.shape}")
        check(self.L.mg3d_ctx_set_coefficient(self._h, P(np.ascontiguousarray(eps).reshape(-1))))

    def has_coefficient(self):
        on = C.c_int(0)
        check(self.L.mg3d_ctx_has_coefficient(self._h, C.byref(on)))
        return bool(on.value)

    def coefficient(self, level=None):
        """eps of a level as the kernels use it, (n, n, n)"""
        level = self.num_levels - 1 if level is None else level
        n = self.level_n(level)
        out = np.empty(n ** 3)
        check(self.L.mg3d_ctx_get_coefficient(self._h, level, P(out)))
        return out.reshape(n, n, n)

    def set_mask(self, mask):
        """mg3d_ctx_set_mask: fixed points inside the domain (embedded conductors).  mask is bool or uint8, (N, N, N) or
        flat, nonzero = fixed: u there keeps what was uploaded and acts as a Dirichlet value, like a point on a Dirichlet
        face; coarser levels take the mask by injection unless set_mask_coarsening("keep") says otherwise.  None: no mask
        again.  Under injection plain cycles are for bodies that survive on the coarse grids, and pcg_solve / wpcg_solve are
        the solvers for thin ones; under "keep" thin bodies stay on every level, plain cycles contract on them and
        fmg_solve accepts the mask.  Rebuilds a coarse factor of get_details();
        drops one given to set_lu.  The bytes are kept as given: a uint8 value 1..255 is a label of its body, which
        field_flux(label) asks for."""
        if mask is None:
            check(self.L.mg3d_ctx_set_mask(self._h, None))
            return
        mask = np.asarray(mask)
        if mask.dtype not in (np.dtype(bool), np.dtype(np.uint8)):
            raise TypeError(f"set_mask: need bool or uint8, got {mask.dtype}")
        if mask.size != self.N ** 3 or mask.shape not in ((self.N ** 3,), (self.N, self.N, self.N)):
            raise ValueError(f"set_mask: need shape ({self.N},)*3 or ({self.N ** 3},), got {mask.shape}")
        m = np.ascontiguousarray(mask).reshape(-1).view(np.uint8)
        check(self.L.mg3d_ctx_set_mask(self._h, m.ctypes.data_as(C.POINTER(C.c_ubyte))))

    def has_mask(self):
        on = C.c_int(0)
        check(self.L.mg3d_ctx_has_mask(self._h, C.byref(on)))
        return bool(on.value)

    def get_mask(self, level=None):
        """the mask of a level as the kernels use it (under either coarsening rule), (n, n, n) uint8"""
        level = self.num_levels - 1 if level is None else level
        n = self.level_n(level)
        out = np.empty(n ** 3, dtype=np.uint8)
        check(self.L.mg3d_ctx_get_mask(self._h, level, out.ctypes.data_as(C.POINTER(C.c_ubyte))))
        return out.reshape(n, n, n)

    def set_mask_coarsening(self, rule):
        """mg3d_ctx_set_mask_coarsening: how the coarser levels take the mask -- "inject" (MG3D_MASK_INJECT = 0, the
        default: m[I,J,K] = m_fine[2I,2J,2K]) or "keep" (MG3D_MASK_KEEP = 1: a fixed point that injection would lose fixes
        its lower parent, so a body thinner than the coarse spacing stays on every level without thickening; it moves by up
        to one fine spacing towards the low index per level).  Operator state: set it before or after the mask, in any order
        with the other setters; a change under a mask rebuilds the coarser masks and the coarse factor of get_details()."""
        if isinstance(rule, str):
            if rule not in MASK_COARSENING:
                raise ValueError(f"set_mask_coarsening: need one of {sorted(MASK_COARSENING)} or the enum value, got {rule!r}")
            rule = MASK_COARSENING[rule]
        check(self.L.mg3d_ctx_set_mask_coarsening(self._h, int(rule)))

    def get_mask_coarsening(self):
        """mg3d_ctx_get_mask_coarsening: the rule by its name, "inject" or "keep", as set_mask_coarsening takes it"""
        rule = C.c_int(0)
        check(self.L.mg3d_ctx_get_mask_coarsening(self._h, C.byref(rule)))
        return {v: k for k, v in MASK_COARSENING.items()}[rule.value]

    def set_shift_field(self, s):
        """mg3d_ctx_set_shift_field: solve  div(eps grad u) - (sigma + s)*u = d  with s >= 0 given at every point of the
        finest level ((N, N, N) or flat float64; coarser levels take it by the context's own restriction, full weighting).
        sigma is set_shift's scalar, eps set_coefficient's or 1.  None: no field again.  Rebuilds a coarse factor of
        get_details(); drops one given to set_lu."""
        if s is None:
            check(self.L.mg3d_ctx_set_shift_field(self._h, None))
            return
        s = np.asarray(s)
        if s.dtype != np.float64:
            raise TypeError(f"set_shift_field: need float64, got {s.dtype}")
        if s.size != self.N ** 3 or s.shape not in ((self.N ** 3,), (self.N, self.N, self.N)):
            raise ValueError(f"set_shift_field: need shape ({self.N},)*3 or ({self.N ** 3},), got {s.shape}")
        check(self.L.mg3d_ctx_set_shift_field(self._h, P(np.ascontiguousarray(s).reshape(-1))))

    def has_shift_field(self):
        on = C.c_int(0)
        check(self.L.mg3d_ctx_has_shift_field(self._h, C.byref(on)))
        return bool(on.value)

    def get_shift_field(self, level=None):
        """the restricted field of a level as the kernels use it, (n, n, n)"""
        level = self.num_levels - 1 if level is None else level
        n = self.level_n(level)
        out = np.empty(n ** 3)
        check(self.L.mg3d_ctx_get_shift_field(self._h, level, P(out)))
        return out.reshape(n, n, n)

    def set_periodic(self, axes):
        """mg3d_ctx_set_periodic: periodic boundaries on the axes given as a mask (MG3D_PERIODIC_I = 1, _J = 2, _K = 4) or
        as an iterable of axis indices 0, 1, 2; 0 or () gives Dirichlet faces everywhere again.  On a periodic axis index
        N-1 duplicates index 0: it is never read and always written as a copy.  With all three axes periodic and sigma = 0
        the operator is singular: u is fixed only up to a constant (the coarse solve pins point (0,0,0) of level 0) and d
        must have zero mean over the unique points, else the residual stalls at that mean -- nothing projects d or u.
        Rebuilds a coarse factor of get_details(); drops one given to set_lu."""
        if not isinstance(axes, (int, np.integer)):
            mask = 0
            for a in axes:
                if a not in (0, 1, 2):
                    raise ValueError(f"set_periodic: axis {a!r} (need 0, 1 or 2)")
                mask |= 1 << int(a)
            axes = mask
        check(self.L.mg3d_ctx_set_periodic(self._h, int(axes)))

    @property
    def periodic(self):
        """the mask of periodic axes"""
        v = C.c_int(0)
        check(self.L.mg3d_ctx_get_periodic(self._h, C.byref(v)))
        return v.value

    def set_neumann(self, faces):
        """mg3d_ctx_set_neumann: homogeneous Neumann faces (du/dn = 0 by reflection) given as a mask (MG3D_NEUMANN_ILO = 1,
        _IHI = 2, _JLO = 4, _JHI = 8, _KLO = 16, _KHI = 32) or as an iterable of names "ilo", "ihi", "jlo", "jhi", "klo",
        "khi"; 0 or () gives none again.  A point on a Neumann face is an unknown unless it also lies on a Dirichlet face.
        An axis is periodic or has Neumann faces, not both.  With sigma = 0 and every axis periodic or Neumann on both faces
        the operator is singular: u is fixed only up to a constant (the coarse solve pins point (0,0,0) of level 0) and d
        must satisfy sum(compatibility_weights() * d) = 0, else the residual stalls -- nothing projects d or u.
        A prescribed flux goes into d with fold_flux().  Rebuilds a coarse factor of get_details(); drops one given to
        set_lu."""
        if not isinstance(faces, (int, np.integer)):
            mask = 0
            for f in faces:
                if f not in NEUMANN_FACES:
                    raise ValueError(f"set_neumann: face {f!r} (need one of {', '.join(NEUMANN_FACES)})")
                mask |= 1 << NEUMANN_FACES.index(f)
            faces = mask
        check(self.L.mg3d_ctx_set_neumann(self._h, int(faces)))

    @property
    def neumann(self):
        """the mask of Neumann faces"""
        v = C.c_int(0)
        check(self.L.mg3d_ctx_get_neumann(self._h, C.byref(v)))
        return v.value

    def compatibility_weights(self):
        """(N, N, N) weights w of the compatibility condition of the singular case: 1/2 per Neumann face a point of the
        finest level lies on (1/4 on an edge of two, 1/8 at a corner of three), 1 elsewhere among the unknowns, 0 at
        Dirichlet points and periodic duplicates.  w is the left null vector of the reflected operator: d is compatible
        when (w * d).sum() == 0; subtract (w * d).sum() / w.sum() from d otherwise."""
        N, per, neu = self.N, self.periodic, self.neumann
        w = np.ones((N, N, N))
        for ax in range(3):
            lo, hi = [slice(None)] * 3, [slice(None)] * 3
            lo[ax], hi[ax] = 0, N - 1
            if (per >> ax) & 1:
                w[tuple(hi)] = 0.
                continue
            for sl, bit in ((lo, 2 * ax), (hi, 2 * ax + 1)):
                w[tuple(sl)] *= 0.5 if (neu >> bit) & 1 else 0.
        return w

    def fold_flux(self, d, flux):
        """mg3d_neumann_fold_flux: folds a prescribed outward normal derivative g = du/dn into the right-hand side d
        ((N, N, N) float64, changed in place and returned) of the finest level: d -= 2 a g / h at each point of each
        Neumann face, a = 1 or, with a coefficient, the mean of eps at the face point and the point inside it.  flux maps
        face names ("ilo" ... "khi") to (N, N) arrays over the face's other two indices in i, j, k order; faces left out
        have g = 0.  Every face named must be a Neumann face of the solver."""
        N = self.N
        if not (isinstance(d, np.ndarray) and d.dtype == np.float64 and d.shape == (N, N, N) and d.flags.c_contiguous):
            raise TypeError(f"fold_flux: d must be a C-contiguous float64 array of shape ({N},)*3")
        faces = self.neumann
        keep, ptrs = [], (dp * 6)()
        for name, g in flux.items():
            if name not in NEUMANN_FACES or not (faces >> NEUMANN_FACES.index(name)) & 1:
                raise ValueError(f"fold_flux: {name!r} is not a Neumann face of this solver")
            g = np.ascontiguousarray(g, dtype=np.float64)
            if g.shape != (N, N):
                raise ValueError(f"fold_flux: flux[{name!r}] needs shape ({N}, {N}), got {g.shape}")
            keep.append(g)
            ptrs[NEUMANN_FACES.index(name)] = P(g)
        eps = np.ascontiguousarray(self.coefficient()).reshape(-1) if self.has_coefficient() else None
        check(self.L.mg3d_neumann_fold_flux(P(d.reshape(-1)), None if eps is None else P(eps), N, self.h, faces, ptrs))
        return d

    def setup_boundary_conditions(self, field=MG3D_D, level=None):
        level = self.num_levels - 1 if level is None else level
        n = self.level_n(level)
        a = self.download(field, level)
        self.L.mg3d_fill_boundary_host(P(a), n, self.level_h(level))
        self.upload(field, level, a)

    def setup_test_problem(self):
        """test_mg_3d.c:11-29: BC values on the faces of d and of u, interior zero."""
        self.get_details()
        self.zero(MG3D_U, self.num_levels - 1)
        self.zero(MG3D_D, self.num_levels - 1)
        self.setup_boundary_conditions(MG3D_D)
        self.setup_boundary_conditions(MG3D_U)

    def get_initial_residual(self):
        return self.l2norm(MG3D_D, self.num_levels - 1)

    def lin_solve(self):
        return self.vcycle(self.num_levels - 1)

    def get_residual(self):
        return self.residual(self.num_levels - 1, store=False)

    # -- data
    def upload(self, field, level, host):
        n = self.level_n(level)
        host = np.ascontiguousarray(host, dtype=np.float64).reshape(-1)
        assert host.size == n ** 3
        check(self.L.mg3d_upload(self._h, field, level, P(host)))

    def download(self, field, level):
        n = self.level_n(level)
        out = np.empty(n ** 3)
        check(self.L.mg3d_download(self._h, field, level, P(out)))
        return out

    def zero(self, field, level):
        check(self.L.mg3d_zero(self._h, field, level))

    def sync(self):
        check(self.L.mg3d_sync(self._h))

    # -- data in device memory: torch tensors on the context's GPU, float64 or float32, any view (include/mg3d.h, "Device
    # arrays").  Ordered on torch's current stream of the tensor's device, no host synchronisation in the first three.
    def upload_tensor(self, field, level, t):
        """mg3d_upload_device: the (n, n, n) tensor t into a field of a level; strides of 0 (expand) are fine.  When the
        call returns t may be overwritten or freed on the current stream."""
        n = self.level_n(level)
        a, stream = _device_args(t, "upload_tensor", (n, n, n))
        check(self.L.mg3d_upload_device(self._h, field, level, C.byref(a), stream))

    def download_tensor(self, field, level, out=None, dtype=None):
        """mg3d_download_device: a field of a level into `out` (any writable (n, n, n) view on the GPU) or into a new
        contiguous tensor of `dtype` (default torch.float64) on the context's device; float32 rounds to nearest.  Work
        enqueued on the current stream afterwards sees the values."""
        import torch
        n = self.level_n(level)
        if out is None:
            if n <= 0:
                raise ValueError(f"download_tensor: bad level {level}")
            out = torch.empty((n, n, n), dtype=torch.float64 if dtype is None else dtype,
                              device=torch.device("cuda", torch.cuda.current_device()))
        a, stream = _device_args(out, "download_tensor", (n, n, n), writable=True)
        check(self.L.mg3d_download_device(self._h, field, level, C.byref(a), stream))
        return out

    def step_set_source_tensor(self, t):
        """mg3d_step_set_source_device: step_set_source from an (N, N, N) tensor on the GPU, no host copy and no host
        synchronisation -- for a source recomputed on the device between step_advance calls.  None drops the source."""
        if t is None:
            check(self.L.mg3d_step_set_source_device(self._h, None, None))
            return
        a, stream = _device_args(t, "step_set_source_tensor", (self.N,) * 3)
        check(self.L.mg3d_step_set_source_device(self._h, C.byref(a), stream))

    def set_mask_tensor(self, t):
        """mg3d_ctx_set_mask_device: set_mask from an (N, N, N) torch.bool or torch.uint8 tensor on the GPU, any view
        (permuted, sliced, expanded); ordered on the tensor's current stream.  None: no mask."""
        if t is None:
            check(self.L.mg3d_ctx_set_mask_device(self._h, None, None))
            return
        import torch
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"set_mask_tensor: need a torch.Tensor, got {type(t).__name__}")
        if t.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f"set_mask_tensor: need torch.bool or torch.uint8, got {t.dtype}")
        if tuple(t.shape) != (self.N,) * 3:
            raise ValueError(f"set_mask_tensor: need shape {(self.N,) * 3}, got {tuple(t.shape)}")
        if not t.is_cuda:
            raise ValueError(f"set_mask_tensor: need a tensor on the GPU, got device {t.device}")
        a = mg3d_array(t.data_ptr(), MG3D_U8, (C.c_longlong * 3)(*t.stride()))
        check(self.L.mg3d_ctx_set_mask_device(self._h, C.byref(a), C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)))

    def set_coefficient_tensor(self, t):
        """mg3d_ctx_set_coefficient_device: set_coefficient from an (N, N, N) tensor on the GPU; checked on the device
        (Mg3dError code 1 names the lowest bad dense index), synchronises with the host.  None: the constant operator."""
        if t is None:
            check(self.L.mg3d_ctx_set_coefficient_device(self._h, None, None))
            return
        a, stream = _device_args(t, "set_coefficient_tensor", (self.N,) * 3)
        check(self.L.mg3d_ctx_set_coefficient_device(self._h, C.byref(a), stream))

    def set_shift_field_tensor(self, t):
        """mg3d_ctx_set_shift_field_device: set_shift_field from an (N, N, N) float64 or float32 tensor on the GPU, any
        view; checked on the device (Mg3dError code 1 names the lowest bad dense index), synchronises with the host.
        None: no field."""
        if t is None:
            check(self.L.mg3d_ctx_set_shift_field_device(self._h, None, None))
            return
        a, stream = _device_args(t, "set_shift_field_tensor", (self.N,) * 3)
        check(self.L.mg3d_ctx_set_shift_field_device(self._h, C.byref(a), stream))

    # -- field output (include/mg3d.h, "Field output"): read-only, the finest level
    def gradient(self, scale=1.0):
        """mg3d_field_gradient: scale * du/dx_a at every point of the finest level, three (N, N, N) float64 arrays for the
        axes i, j, k (scale=-1: E).  Periodic wraps, reflected Neumann faces, one-sided differences on Dirichlet faces; the
        mask is ignored."""
        N = self.N
        out = [np.empty(N ** 3) for _ in range(3)]
        check(self.L.mg3d_field_gradient(self._h, float(scale), P(out[0]), P(out[1]), P(out[2])))
        return tuple(a.reshape(N, N, N) for a in out)

    def gradient_tensor(self, out=None, dtype=None, scale=1.0):
        """mg3d_field_gradient_device: the same into GPU tensors, one launch for all wanted components, ordered on the
        current stream, no host synchronisation.  out=None: a new (3, N, N, N) tensor of `dtype` (default torch.float64) on
        the context's device; else a (3, N, N, N)-shaped tensor (any view) or a sequence of three (N, N, N) tensors or None
        (component not wanted), float64 or float32 each.  Returns out."""
        import torch
        N = self.N
        if out is None:
            out = torch.empty((3, N, N, N), dtype=torch.float64 if dtype is None else dtype,
                              device=torch.device("cuda", torch.cuda.current_device()))
        if isinstance(out, torch.Tensor):
            if tuple(out.shape) != (3, N, N, N):
                raise ValueError(f"gradient_tensor: need shape {(3, N, N, N)}, got {tuple(out.shape)}")
            parts = [out[0], out[1], out[2]]
        else:
            parts = list(out)
            if len(parts) != 3:
                raise ValueError(f"gradient_tensor: need three components, got {len(parts)}")
        descs, stream = [None] * 3, None
        for a, t in enumerate(parts):
            if t is not None:
                descs[a], st = _device_args(t, "gradient_tensor", (N, N, N), writable=True)
                stream = st if stream is None else stream
        ptrs = (_ap * 3)(*[C.pointer(d) if d is not None else _ap() for d in descs])
        check(self.L.mg3d_field_gradient_device(self._h, float(scale), ptrs, stream))
        return out

    def field_flux(self, label=0):
        """mg3d_field_flux: h * the sum of w(p)*(s - D*u_p) over the fixed unknowns whose mask byte is `label` (0: all) --
        the net flux of eps grad u into that body for a converged solution; times -eps_0 its charge."""
        f = C.c_double(0.)
        check(self.L.mg3d_field_flux(self._h, int(label), C.byref(f)))
        return f.value

    def field_energy(self):
        """mg3d_field_energy: 0.5 * h * the sum over the grid edges of w_e * a_e * (u_q - u_p)^2."""
        w = C.c_double(0.)
        check(self.L.mg3d_field_energy(self._h, C.byref(w)))
        return w.value

    # -- particles (include/mg3d.h, "Particles"): gather at points, scatter of point charges; the finest level
    def sample(self, xyz, scale=1.0):
        """mg3d_field_sample: u and scale * grad u at the points xyz ((M, 3) float64: x along i, y along j, z along k),
        trilinear in the nodal values, NaN for a point outside the box.  Returns (u (M,), grad (M, 3))."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float64)
        if xyz.ndim != 2 or xyz.shape[1] != 3:
            raise ValueError(f"sample: positions need shape (M, 3), got {xyz.shape}")
        M = xyz.shape[0]
        u, g = np.empty(M), np.empty((M, 3))
        check(self.L.mg3d_field_sample(self._h, M, P(xyz.reshape(-1)), float(scale), P(u), P(g.reshape(-1))))
        return u, g

    def deposit(self, xyz, q, scale=1.0):
        """mg3d_deposit: d of the finest level += scale * (cloud-in-cell density of the charges q (M,) at xyz (M, 3)),
        doubled per Neumann face a node lies on.  Deterministic and independent of the order of the points."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float64)
        q = np.ascontiguousarray(q, dtype=np.float64)
        if xyz.ndim != 2 or xyz.shape[1] != 3:
            raise ValueError(f"deposit: positions need shape (M, 3), got {xyz.shape}")
        if q.shape != (xyz.shape[0],):
            raise ValueError(f"deposit: q needs shape ({xyz.shape[0]},), got {q.shape}")
        check(self.L.mg3d_deposit(self._h, xyz.shape[0], P(xyz.reshape(-1)), P(q), float(scale)))

    def sample_tensor(self, pos, want_u=True, want_grad=True, scale=1.0, out_u=None, out_grad=None, dtype=None):
        """mg3d_field_sample_device: the same on GPU tensors, one launch, ordered on the current stream, no host
        synchronisation.  pos is an (M, 3) tensor (any view) or a sequence of three 1-D tensors, float64 or float32.
        out_u (M,) / out_grad (M, 3) (any writable views) are written when given, else new tensors of `dtype` (default
        torch.float64) are made for what want_u / want_grad ask for.  Returns (u or None, grad or None)."""
        import torch
        descs, M, dev, stream = _position_args(pos, "sample_tensor")
        dt = torch.float64 if dtype is None else dtype
        if out_u is None and want_u:
            out_u = torch.empty((M,), dtype=dt, device=dev)
        if out_grad is None and want_grad:
            out_grad = torch.empty((M, 3), dtype=dt, device=dev)
        du, dg = None, [None] * 3
        if out_u is not None:
            if not (isinstance(out_u, torch.Tensor) and out_u.is_cuda and out_u.device == dev):
                raise ValueError(f"sample_tensor: out_u must be a tensor on {dev}")
            if tuple(out_u.shape) != (M,):
                raise ValueError(f"sample_tensor: out_u needs shape ({M},), got {tuple(out_u.shape)}")
            du = vec_desc(out_u, writable=True, count=M)
        if out_grad is not None:
            if not (isinstance(out_grad, torch.Tensor) and out_grad.is_cuda and out_grad.device == dev):
                raise ValueError(f"sample_tensor: out_grad must be a tensor on {dev}")
            if tuple(out_grad.shape) != (M, 3):
                raise ValueError(f"sample_tensor: out_grad needs shape ({M}, 3), got {tuple(out_grad.shape)}")
            dg = [vec_desc(out_grad[:, a], writable=True, count=M) for a in range(3)]
        check(self.L.mg3d_field_sample_device(self._h, M, _vec_ptrs(descs), float(scale),
                                              C.byref(du) if du is not None else None, _vec_ptrs(dg), stream))
        return out_u, out_grad

    def deposit_tensor(self, pos, q, scale=1.0):
        """mg3d_deposit_device: deposit() from GPU tensors -- pos as in sample_tensor, q an (M,) tensor, float64 or
        float32, any view (expand: one charge for all) --, ordered on the current stream, no host synchronisation."""
        import torch
        descs, M, dev, stream = _position_args(pos, "deposit_tensor")
        if not (isinstance(q, torch.Tensor) and q.is_cuda and q.device == dev):
            raise ValueError(f"deposit_tensor: q must be a tensor on {dev}")
        if tuple(q.shape) != (M,):
            raise ValueError(f"deposit_tensor: q needs shape ({M},), got {tuple(q.shape)}")
        dq = vec_desc(q, count=M)
        check(self.L.mg3d_deposit_device(self._h, M, _vec_ptrs(descs), C.byref(dq), float(scale), stream))

    @staticmethod
    def _push_params(dt, scale, accel, drag):
        accel = tuple(float(a) for a in accel)
        if len(accel) != 3:
            raise ValueError(f"push: accel needs three components, got {len(accel)}")
        return mg3d_push_params(float(dt), float(scale), (C.c_double * 3)(*accel), float(drag))

    def push_tensor(self, pos, vel, qm, dt, fate, scale=-1.0, accel=(0., 0., 0.), drag=0.0):
        """mg3d_particle_push_device: one kick-and-drift step, in place, of the particles whose fate is 0 --
        v = (v + (qm*dt)*E + dt*accel) / (1 + drag*dt), x += dt*v with E = scale * grad u gathered as sample_tensor
        gathers it -- with the context's walls (periodic axes wrap, Neumann faces reflect, Dirichlet faces retire) and
        conductors (a nonzero mask byte at the nearest node retires with that label).  pos (float64) and vel (float64 or
        float32) are each an (M, 3) tensor (any view) or three 1-D tensors; qm an (M,) tensor or a Python float (one value
        for all); fate an (M,) torch.int32 tensor of MG3D_FATE_* values.  One launch on the current stream, no host
        synchronisation; push_counts() has the running totals."""
        import torch
        dpos, M, dev, stream = _position_args(pos, "push_tensor", writable=True)
        dvel, Mv, devv, _ = _position_args(vel, "push_tensor", writable=True)
        if Mv != M or devv != dev:
            raise ValueError(f"push_tensor: {M} positions on {dev}, {Mv} velocities on {devv}")
        if any(d.dtype != MG3D_F64 for d in dpos):
            raise TypeError("push_tensor: positions need float64")
        if not isinstance(qm, torch.Tensor):
            qm = torch.tensor([float(qm)], dtype=torch.float64, device=dev).expand(M)
        if not (qm.is_cuda and qm.device == dev):
            raise ValueError(f"push_tensor: qm must be a tensor on {dev}")
        if tuple(qm.shape) != (M,):
            raise ValueError(f"push_tensor: qm needs shape ({M},), got {tuple(qm.shape)}")
        if not (isinstance(fate, torch.Tensor) and fate.is_cuda and fate.device == dev):
            raise ValueError(f"push_tensor: fate must be a tensor on {dev}")
        dq = vec_desc(qm, count=M)
        df = vec_desc(fate, count=M, fate=True)
        pp = self._push_params(dt, scale, accel, drag)
        check(self.L.mg3d_particle_push_device(self._h, M, _vec_ptrs(dpos), _vec_ptrs(dvel), C.byref(dq), C.byref(df),
                                               C.byref(pp), stream))

    def push(self, xyz, vel, qm, dt, fate=None, scale=-1.0, accel=(0., 0., 0.), drag=0.0):
        """mg3d_particle_push: push_tensor on numpy arrays -- xyz and vel (M, 3), qm (M,) or a float, fate (M,) int32 or
        None (all alive).  Returns new arrays (xyz, vel, fate)."""
        xyz = np.array(xyz, dtype=np.float64, order="C")
        vel = np.array(vel, dtype=np.float64, order="C")
        if xyz.ndim != 2 or xyz.shape[1] != 3 or vel.shape != xyz.shape:
            raise ValueError(f"push: positions and velocities need one shape (M, 3), got {xyz.shape} and {vel.shape}")
        M = xyz.shape[0]
        qm = np.ascontiguousarray(np.broadcast_to(np.asarray(qm, dtype=np.float64), (M,)))
        fate = np.zeros(M, dtype=np.int32) if fate is None else np.array(fate, dtype=np.int32, order="C")
        if fate.shape != (M,):
            raise ValueError(f"push: fate needs shape ({M},), got {fate.shape}")
        pp = self._push_params(dt, scale, accel, drag)
        check(self.L.mg3d_particle_push(self._h, M, P(xyz.reshape(-1)), P(vel.reshape(-1)), P(qm),
                                        fate.ctypes.data_as(C.POINTER(C.c_int)), C.byref(pp)))
        return xyz, vel, fate

    def push_counts(self, reset=False):
        """mg3d_particle_counts: how many particles each fate has taken since the context was made (or since the last
        reset), a (MG3D_FATE_SLOTS,) uint64 array indexed by fate; one host synchronisation."""
        out = np.zeros(MG3D_FATE_SLOTS, dtype=np.uint64)
        check(self.L.mg3d_particle_counts(self._h, out.ctypes.data_as(C.POINTER(C.c_ulonglong)), int(bool(reset))))
        return out

    def sort_tensor(self, pos, fate=None, shift=0, out=None):
        """mg3d_particle_sort_device: the stable permutation that puts the particles in cell order (blocks of 2**shift
        cells per side), the lost behind the living and the dead (fate != 0) last.  pos as in sample_tensor, fate an (M,)
        torch.int32 tensor (any view) or None: all alive.  Returns (perm, counts): perm an (M,) int32 tensor -- `out` when
        given, any view of stride >= 1 -- with perm[m] the old index of the particle that belongs at place m, counts a
        (2,) int64 tensor (inside, lost), both on the GPU.  Ordered on the current stream, no host synchronisation."""
        import torch
        descs, M, dev, stream = _position_args(pos, "sort_tensor")
        df = None
        if fate is not None:
            if not (isinstance(fate, torch.Tensor) and fate.is_cuda and fate.device == dev):
                raise ValueError(f"sort_tensor: fate must be a tensor on {dev}")
            if fate.dtype != torch.int32:
                raise TypeError(f"sort_tensor: fate is int32, got {fate.dtype}")
            df = _data_vec(fate, "sort_tensor", count=M)
        if out is None:
            out = torch.empty((M,), dtype=torch.int32, device=dev)
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == dev):
            raise ValueError(f"sort_tensor: out must be a tensor on {dev}")
        if out.dtype != torch.int32:
            raise TypeError(f"sort_tensor: the permutation is int32, got {out.dtype}")
        dp_ = _data_vec(out, "sort_tensor", writable=True, count=M)
        counts = torch.zeros((2,), dtype=torch.int64, device=dev)
        check(self.L.mg3d_particle_sort_device(self._h, M, _vec_ptrs(descs), C.byref(df) if df is not None else None,
                                               int(shift), C.byref(dp_), C.c_void_p(counts.data_ptr()), stream))
        return out, counts

    def permute_tensors(self, perm, *tensors):
        """mg3d_particle_permute_device: new tensors t[perm] for every t of `tensors` -- each (M,) or (M, 3), float64,
        float32 or int32, any view; an (M, 3) tensor counts as three vectors -- with up to MG3D_PERMUTE_MAX_VECS vectors
        per launch, the bytes copied as they are.  perm: an (M,) int32 tensor.  An entry of perm outside 0..M-1 leaves its
        element of the outputs unwritten.  Ordered on the current stream, no host synchronisation."""
        import torch
        if not (isinstance(perm, torch.Tensor) and perm.is_cuda):
            raise ValueError("permute_tensors: perm must be a tensor on the GPU")
        if perm.dtype != torch.int32:
            raise TypeError(f"permute_tensors: the permutation is int32, got {perm.dtype}")
        dev = perm.device
        dperm = _data_vec(perm, "permute_tensors")
        M = perm.shape[0]
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        outs, src, dst = [], [], []
        for t in tensors:
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == dev):
                raise ValueError(f"permute_tensors: every tensor must be on {dev}")
            if not (tuple(t.shape) == (M,) or tuple(t.shape) == (M, 3)):
                raise ValueError(f"permute_tensors: need shape ({M},) or ({M}, 3), got {tuple(t.shape)}")
            o = torch.empty(t.shape, dtype=t.dtype, device=dev)
            outs.append(o)
            for a, b in ([(t, o)] if t.dim() == 1 else [(t[:, k], o[:, k]) for k in range(3)]):
                src.append(_data_vec(a, "permute_tensors", count=M))
                dst.append(_data_vec(b, "permute_tensors", writable=True, count=M))
        for lo in range(0, len(src), MG3D_PERMUTE_MAX_VECS):
            n = min(MG3D_PERMUTE_MAX_VECS, len(src) - lo)
            ps = (_vp * n)(*[C.pointer(d) for d in src[lo:lo + n]])
            pd = (_vp * n)(*[C.pointer(d) for d in dst[lo:lo + n]])
            check(self.L.mg3d_particle_permute_device(self._h, M, C.byref(dperm), n, ps, pd, stream))
        return tuple(outs)

    def sort(self, xyz, fate=None, shift=0):
        """mg3d_particle_sort: sort_tensor on numpy arrays -- xyz (M, 3), fate (M,) int32 or None.  Returns
        (perm (M,) int32, (n_inside, n_lost)); one host synchronisation."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float64)
        if xyz.ndim != 2 or xyz.shape[1] != 3:
            raise ValueError(f"sort: positions need shape (M, 3), got {xyz.shape}")
        M = xyz.shape[0]
        pf = None
        if fate is not None:
            fate = np.ascontiguousarray(fate, dtype=np.int32)
            if fate.shape != (M,):
                raise ValueError(f"sort: fate needs shape ({M},), got {fate.shape}")
            pf = fate.ctypes.data_as(C.POINTER(C.c_int))
        perm = np.empty(M, dtype=np.int32)
        counts = (C.c_longlong * 2)(0, 0)
        check(self.L.mg3d_particle_sort(self._h, M, P(xyz.reshape(-1)), pf, int(shift),
                                        perm.ctypes.data_as(C.POINTER(C.c_int)), counts))
        return perm, (int(counts[0]), int(counts[1]))

    # -- operators
    def smooth(self, level, post, iters):
        check(self.L.mg3d_smooth(self._h, level, int(post), iters))

    def residual(self, level, store=True, want_norm=True):
        nrm = C.c_double(0)
        check(self.L.mg3d_residual(self._h, level, int(store), C.byref(nrm) if want_norm else None))
        return nrm.value

    def smooth_residual(self, level, post, iters, store=True, want_norm=True):
        nrm = C.c_double(0)
        check(self.L.mg3d_smooth_residual(self._h, level, int(post), iters, int(store),
                                          C.byref(nrm) if want_norm else None))
        return nrm.value

    def smooth_restrict(self, level, iters):
        check(self.L.mg3d_smooth_restrict(self._h, level, iters))

    def restrict(self, level):
        check(self.L.mg3d_restrict(self._h, level))

    def prolong(self, level):
        check(self.L.mg3d_prolong(self._h, level))

    def coarse_solve(self):
        check(self.L.mg3d_coarse_solve(self._h))

    def l2norm(self, field, level):
        nrm = C.c_double(0)
        check(self.L.mg3d_l2norm(self._h, field, level, C.byref(nrm)))
        return nrm.value

    def vcycle(self, level=None, want_norm=True):
        level = self.num_levels - 1 if level is None else level
        nrm = C.c_double(0)
        check(self.L.mg3d_vcycle(self._h, level, C.byref(nrm) if want_norm else None))
        return nrm.value

    def vcycles(self, count):
        norms = np.zeros(count)
        check(self.L.mg3d_vcycles(self._h, count, P(norms)))
        return norms

    def pcg_solve(self, rtol=1e-8, atol=0.0, max_iters=50):
        """mg3d_pcg_solve: conjugate gradients preconditioned by one V-cycle per iteration, from the uploaded u and d of the
        finest level until ||r|| <= max(rtol * ||r_0||, atol).  Returns (norms ||r_0|| .. ||r_iterations||, info dict:
        iterations, converged, r0_norm, r_norm).  For coefficients that jump; not with Neumann faces or the singular
        all-periodic case (Mg3dError, code 5): wpcg_solve."""
        norms = np.zeros(max(int(max_iters), 0) + 1)
        info = PcgInfo()
        check(self.L.mg3d_pcg_solve(self._h, float(rtol), float(atol), int(max_iters), P(norms), C.byref(info)))
        return norms[:info.iterations + 1].copy(), {"iterations": info.iterations, "converged": bool(info.converged),
                                                    "r0_norm": info.r0_norm, "r_norm": info.r_norm}

    def wpcg_solve(self, rtol=1e-8, atol=0.0, max_iters=50):
        """mg3d_wpcg_solve: pcg_solve in the inner product weighted by compatibility_weights(), for contexts with Neumann
        faces and for the singular operator (every axis periodic or Neumann on both faces, sigma = 0), which is solved on
        the subspace of w-mean zero; on any other context it is pcg_solve, bit for bit.  Returns (norms, info dict:
        iterations, converged, r0_norm, r_norm, singular, rhs_mean -- the w-mean of d that was projected out)."""
        norms = np.zeros(max(int(max_iters), 0) + 1)
        info = WpcgInfo()
        check(self.L.mg3d_wpcg_solve(self._h, float(rtol), float(atol), int(max_iters), P(norms), C.byref(info)))
        return norms[:info.iterations + 1].copy(), {"iterations": info.iterations, "converged": bool(info.converged),
                                                    "r0_norm": info.r0_norm, "r_norm": info.r_norm,
                                                    "singular": bool(info.singular), "rhs_mean": info.rhs_mean}

    def fmg_initialize(self):
        check(self.L.mg3d_fmg_initialize(self._h))

    def fmg_interpolate(self, level):
        """mg3d_fmg_interpolate: every unknown of u[level] overwritten with the cubic interpolant of u[level - 1]
        (1 <= level < num_levels); Dirichlet points stay, and so do the fixed points of a mask (accepted under
        set_mask_coarsening("keep") only)."""
        check(self.L.mg3d_fmg_interpolate(self._h, int(level)))

    def fmg_solve(self, cycles=1):
        """mg3d_fmg_solve: full multigrid from the uploaded d and the Dirichlet points of the uploaded u of the finest
        level (its interior is ignored) -- d restricted down the hierarchy, a direct solve, then per level the cubic
        interpolant as the guess of `cycles` V-cycles that keep it.  With V(2,2) one cycle per level leaves an algebraic
        error below the discretisation error.  With a mask (under set_mask_coarsening("keep") only; under "inject" the
        call raises MG3D_ERR_STATE) the fixed points of the uploaded u are read as the Dirichlet points are, and every
        level's body carries its conductor's potential; d at fixed points is never read.  Returns the residual norm after
        the last finest-level cycle."""
        nrm = C.c_double(0)
        check(self.L.mg3d_fmg_solve(self._h, int(cycles), C.byref(nrm)))
        return nrm.value

    # -- implicit time stepping, csrc/mg3d_step.hip
    def step_setup(self, dt, theta=1.0, kappa=0.0):
        """mg3d_step_setup: the theta-scheme (1: backward Euler, 0.5: Crank-Nicolson) for
        u_t = div(eps grad u) - kappa*u + s with steps of dt.  Sets the shift to kappa + 1/(theta*dt) as set_shift does."""
        check(self.L.mg3d_step_setup(self._h, float(dt), float(theta), float(kappa)))

    def step_set_source(self, s):
        """mg3d_step_set_source: the source s of the finest level ((N, N, N) or flat float64), kept on the device; None
        drops it.  May be called between step_advance calls."""
        if s is None:
            check(self.L.mg3d_step_set_source(self._h, None))
            return
        s = np.asarray(s)
        if s.dtype != np.float64:
            raise TypeError(f"step_set_source: need float64, got {s.dtype}")
        if s.size != self.N ** 3 or s.shape not in ((self.N ** 3,), (self.N, self.N, self.N)):
            raise ValueError(f"step_set_source: need shape ({self.N},)*3 or ({self.N ** 3},), got {s.shape}")
        check(self.L.mg3d_step_set_source(self._h, P(np.ascontiguousarray(s).reshape(-1))))

    def step_advance(self, nsteps, cycles=2, method="vcycles", rtol=1e-8):
        """mg3d_step_advance: nsteps steps from u of the finest level, entirely on the device; each step forms its
        right-hand side in one launch and solves with `cycles` V-cycles (method "vcycles") or with wpcg_solve(rtol,
        max_iters=cycles) (method "wpcg"), warm-started from the previous step.  Returns (one norm per step, info dict:
        steps, iterations, converged, time)."""
        if method not in STEP_METHODS:
            raise ValueError(f"step_advance: method {method!r} (need one of {', '.join(STEP_METHODS)})")
        norms = np.zeros(max(int(nsteps), 0))
        info = StepInfo()
        check(self.L.mg3d_step_advance(self._h, int(nsteps), STEP_METHODS[method], int(cycles), float(rtol), P(norms),
                                       C.byref(info)))
        return norms, {"steps": info.steps, "iterations": info.iterations, "converged": bool(info.converged),
                       "time": info.time}

    # -- nonlinear solves, csrc/mg3d_nl.hip
    def nl_setup(self, kind, g0=1.0, beta=1.0, uref=0.0):
        """mg3d_nl_setup: the nonlinear term of  A u - g0*g*phi(beta*(u - uref)) = d,  phi = exp (kind "exp", Boltzmann
        electrons) or sinh (kind "sinh", Poisson-Boltzmann); g0 >= 0, beta > 0."""
        if kind not in NL_KINDS:
            raise ValueError(f"nl_setup: kind {kind!r} (need one of {', '.join(NL_KINDS)})")
        check(self.L.mg3d_nl_setup(self._h, NL_KINDS[kind], float(g0), float(beta), float(uref)))

    def nl_set_weight(self, g):
        """mg3d_nl_set_weight: the weight g >= 0 of the finest level ((N, N, N) or flat float64), kept on the device;
        None drops it (g = 1 everywhere)."""
        if g is None:
            check(self.L.mg3d_nl_set_weight(self._h, None))
            return
        g = np.asarray(g)
        if g.dtype != np.float64:
            raise TypeError(f"nl_set_weight: need float64, got {g.dtype}")
        if g.size != self.N ** 3 or g.shape not in ((self.N ** 3,), (self.N, self.N, self.N)):
            raise ValueError(f"nl_set_weight: need shape ({self.N},)*3 or ({self.N ** 3},), got {g.shape}")
        check(self.L.mg3d_nl_set_weight(self._h, P(np.ascontiguousarray(g).reshape(-1))))

    def nl_set_weight_tensor(self, t):
        """mg3d_nl_set_weight_device: nl_set_weight from an (N, N, N) float64 or float32 tensor on the GPU, any view, no
        host copy.  None drops the weight."""
        if t is None:
            check(self.L.mg3d_nl_set_weight_device(self._h, None, None))
            return
        a, stream = _device_args(t, "nl_set_weight_tensor", (self.N,) * 3)
        check(self.L.mg3d_nl_set_weight_device(self._h, C.byref(a), stream))

    def nl_residual(self, store=False):
        """mg3d_nl_residual: ||F||, F = d - (A u - g0*g*phi(beta*(u - uref))) at the unknowns of the finest level; with
        store, F goes into r of that level."""
        nrm = C.c_double()
        check(self.L.mg3d_nl_residual(self._h, int(bool(store)), C.byref(nrm)))
        return nrm.value

    def nl_solve(self, max_newton=20, cycles=2, method="vcycles", rtol_lin=1e-2, rtol=1e-8, atol=0.0, max_halvings=10):
        """mg3d_nl_solve: damped Newton-multigrid from u of the finest level, entirely on the device: each step evaluates
        the residual and the linearisation in one launch, installs it as the screening field, solves the correction with
        `cycles` V-cycles (method "vcycles") or wpcg_solve(rtol_lin, max_iters=cycles) (method "wpcg") and backtracks on
        ||F||.  Returns (norms[0 .. iterations], info dict: iterations, converged, halvings, linear_iterations,
        last_lambda, norm0, norm).  Afterwards the context holds the linearisation at u (has_shift_field() is True;
        set_shift_field(None) drops it)."""
        if method not in STEP_METHODS:
            raise ValueError(f"nl_solve: method {method!r} (need one of {', '.join(STEP_METHODS)})")
        norms = np.zeros(max(int(max_newton), 0) + 1)
        info = NlInfo()
        check(self.L.mg3d_nl_solve(self._h, int(max_newton), STEP_METHODS[method], int(cycles), float(rtol_lin), float(rtol),
                                   float(atol), int(max_halvings), P(norms), C.byref(info)))
        return norms[:info.iterations + 1], {"iterations": info.iterations, "converged": bool(info.converged),
                                             "halvings": info.halvings, "linear_iterations": info.linear_iterations,
                                             "last_lambda": info.last_lambda, "norm0": info.norm0, "norm": info.norm}

    # -- the mixed-boundary ("electrospray") problem, csrc/mg3d_es.hip
    def es_setup(self, params=None):
        self.es = params or EsParams.default()
        check(self.L.mg3d_es_setup(self._h, C.byref(self.es)))
        return self.es

    def es_smooth(self, level, post, iters):
        check(self.L.mg3d_es_smooth(self._h, level, int(post), iters))

    def es_vcycles(self, count):
        norms = np.zeros(count)
        check(self.L.mg3d_es_vcycles(self._h, count, P(norms)))
        return norms

    def fill_boundary(self, field, level):
        check(self.L.mg3d_fill_boundary(self._h, field, level))

    # -- timing
    def timing_enable(self, on=True):
        check(self.L.mg3d_timing_enable(self._h, int(on)))

    def timing_reset(self):
        check(self.L.mg3d_timing_reset(self._h))

    def kernel_times(self):
        out = {}
        for l in range(self.num_levels):
            for k in range(64):  # up to MG3D_NUM_KERNELS: the library names the ones it has
                if self.L.mg3d_kernel_name(k) == b"?":
                    break
                calls, secs = C.c_int(0), C.c_double(0)
                check(self.L.mg3d_kernel_time_get(self._h, l, k, C.byref(calls), C.byref(secs)))
                if calls.value:
                    out[(l, self.L.mg3d_kernel_name(k).decode())] = (calls.value, secs.value)
        return out

    def timing(self):
        out = {}
        for l in range(self.num_levels):
            for s in range(STAGES):
                calls, secs = C.c_int(0), C.c_double(0)
                check(self.L.mg3d_timing_get(self._h, l, s, C.byref(calls), C.byref(secs)))
                out[(l, self.L.mg3d_stage_name(s).decode())] = (calls.value, secs.value)
        return out


class DistSolver:
    """V-cycle on i-slabs: rank `rank` of `nranks` (one process per GPU, RCCL), or -- unique_id=None -- all ranks
    virtual in this process on one GPU (loopback transport; used to verify the decomposition)."""

    def __init__(self, coarse_pts, num_levels, smooth_iters, rank=0, nranks=1, unique_id=None, device=0,
                 grid_length=1.0):
        self.L = lib()
        self._h = C.c_void_p()
        uid = None if unique_id is None else C.c_char_p(bytes(unique_id))
        check(self.L.mg3d_dist_create(coarse_pts, num_levels, smooth_iters, grid_length, rank, nranks, uid, device,
                                      C.byref(self._h)))
        self.c, self.num_levels, self.nu, self.rank, self.nranks = coarse_pts, num_levels, smooth_iters, rank, nranks
        self.N = (coarse_pts - 1) * (1 << (num_levels - 1)) + 1
        self.h = grid_length / (self.N - 1)
        self.first_level = self.L.mg3d_dist_first_level(self._h)
        self.halo = self.L.mg3d_dist_halo(self._h)

    def carried_cycles(self):
        return self.L.mg3d_dist_carried_cycles(self._h)

    def legs_cycles(self):
        return self.L.mg3d_dist_legs_cycles(self._h)

    def comm_info(self):
        """(ranks in the RCCL communicator, overlap on/off, HIP device)"""
        n, ov, dev = C.c_int(0), C.c_int(0), C.c_int(0)
        check(self.L.mg3d_dist_comm_info(self._h, C.byref(n), C.byref(ov), C.byref(dev)))
        return n.value, bool(ov.value), dev.value

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        check(lib().mg3d_comm_unique_id(buf))
        return buf.raw

    def close(self):
        if self._h:
            check(self.L.mg3d_dist_destroy(self._h))
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

    def level_n(self, level):
        return (self.c - 1) * (1 << level) + 1

    def set_keep_residual(self, keep=True):
        check(self.L.mg3d_dist_set_keep_residual(self._h, int(keep)))

    def set_option(self, key, value):
        check(self.L.mg3d_dist_set_option(self._h, key.encode(), int(value)))

    def set_shift(self, sigma):
        """mg3d_dist_set_shift: the screened operator on every local rank (every rank of a job passes the same sigma)."""
        check(self.L.mg3d_dist_set_shift(self._h, float(sigma)))

    def set_coefficient(self, eps):
        """mg3d_dist_set_coefficient: div(eps grad u) - sigma*u = d on every local rank.  eps as Solver.set_coefficient:
        the FULL finest level, (N, N, N) or flat float64; every rank of a job passes the same array.  None: the constant
        operator and its schedules again."""
        if eps is None:
            check(self.L.mg3d_dist_set_coefficient(self._h, None))
            return
        eps = np.asarray(eps)
        if eps.dtype != np.float64:
            raise TypeError(f"set_coefficient: need float64, got {eps.dtype}")
        if eps.size != self.N ** 3 or eps.shape not in ((self.N ** 3,), (self.N, self.N, self.N)):
            raise ValueError(f"set_coefficient: need shape ({self.N},)*3 or ({self.N ** 3},), got {eps.shape}")
        check(self.L.mg3d_dist_set_coefficient(self._h, P(np.ascontiguousarray(eps).reshape(-1))))

    def has_coefficient(self):
        on = C.c_int(0)
        check(self.L.mg3d_dist_has_coefficient(self._h, C.byref(on)))
        return bool(on.value)

    def coefficient(self, level=None):
        """eps of a level as the kernels use it, (n, n, n): the planes the local ranks own (every plane of a replicated
        level, or with the loopback transport); zero elsewhere"""
        level = self.num_levels - 1 if level is None else level
        n = self.level_n(level)
        out = np.zeros(n ** 3)
        check(self.L.mg3d_dist_get_coefficient(self._h, level, P(out)))
        return out.reshape(n, n, n)

    def setup_test_problem(self):
        """test_mg_3d.c:11-29 on the full grid; every rank takes its slab."""
        check(self.L.mg3d_dist_build_coarse(self._h, self.h * (1 << (self.num_levels - 1))))
        full = np.zeros(self.N ** 3)
        self.L.mg3d_fill_boundary_host(P(full), self.N, self.h)
        fin = self.num_levels - 1
        self.upload(MG3D_D, fin, full)
        self.upload(MG3D_U, fin, full)
        return float(np.sqrt((full * full).sum()))

    def upload(self, field, level, host_full):
        host_full = np.ascontiguousarray(host_full, dtype=np.float64).reshape(-1)
        assert host_full.size == self.level_n(level) ** 3
        check(self.L.mg3d_dist_upload(self._h, field, level, P(host_full)))

    def download(self, field, level, out=None):
        n = self.level_n(level)
        out = np.zeros(n ** 3) if out is None else out
        check(self.L.mg3d_dist_download(self._h, field, level, P(out)))
        return out

    def vcycles(self, count):
        norms = np.zeros(count)
        check(self.L.mg3d_dist_vcycles(self._h, count, P(norms)))
        return norms

    def sync(self):
        check(self.L.mg3d_dist_sync(self._h))

    def timing_enable(self, on=True):
        check(self.L.mg3d_dist_timing_enable(self._h, int(on)))

    def timing(self):
        """per-cycle means since timing_enable(True): whole cycle, exchanges the compute stream waits for at once
        (critical path), exchanges that run overlapped (the u halos, underneath the launches in between), the
        replicated / rank-0 coarse levels; kernels on the distributed levels are what is left of the cycle"""
        ms = (C.c_double * 4)()
        n = C.c_int(0)
        check(self.L.mg3d_dist_timing_get(self._h, ms, C.byref(n)))
        k = max(1, n.value)
        return {"cycles": n.value, "cycle_ms": ms[0] / k, "exchange_ms": ms[1] / k, "exchange_overlapped_ms": ms[2] / k,
                "replicated_ms": ms[3] / k, "kernels_ms": (ms[0] - ms[1] - ms[3]) / k}


def PF(a):
    if a is None:
        return None
    assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"], "need contiguous float32"
    return a.ctypes.data_as(fp)


class Solver32:
    """The single-precision / damped-Jacobi / F-cycle variant (BASELINE configs[4]; parity unpinned: semantics in
    csrc/mg3d_f32.hip, restated in plain C by the test infrastructure).  Same field and level numbering as `Solver`."""

    def __init__(self, coarse_pts, num_levels, smooth_iters, omega=6.0 / 7.0, grid_length=1.0):
        self.L = lib()
        self._h = C.c_void_p()
        check(self.L.mg3d32_create(coarse_pts, num_levels, smooth_iters, omega, grid_length, C.byref(self._h)))
        self.c, self.num_levels, self.nu, self.omega = coarse_pts, num_levels, smooth_iters, omega
        self.N = (coarse_pts - 1) * (1 << (num_levels - 1)) + 1

    def close(self):
        if self._h:
            self.L.mg3d32_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_option(self, key, value):
        """mg3d32_set_option: "pairs", "fuse", "carry" (1 on, 0 off)."""
        check(self.L.mg3d32_set_option(self._h, key.encode(), int(value)))

    def timing_enable(self, on=True):
        check(self.L.mg3d32_timing_enable(self._h, int(on)))

    def kernel_times(self):
        """{kernel name: (launches, seconds)} of the finest level's launches since timing_enable(True)"""
        out, k = {}, 0
        while self.L.mg3d32_kernel_name(k):
            n, sec = C.c_int(0), C.c_double(0)
            check(self.L.mg3d32_kernel_time_get(self._h, k, C.byref(n), C.byref(sec)))
            if n.value:
                out[self.L.mg3d32_kernel_name(k).decode()] = (n.value, sec.value)
            k += 1
        return out

    def level_n(self, level):
        return self.L.mg3d32_level_n(self._h, level)

    def upload(self, field, level, host):
        n = self.level_n(level)
        assert host.size == n ** 3
        check(self.L.mg3d32_upload(self._h, field, level, PF(np.ascontiguousarray(host, dtype=np.float32))))

    def download(self, field, level):
        out = np.empty(self.level_n(level) ** 3, dtype=np.float32)
        check(self.L.mg3d32_download(self._h, field, level, PF(out)))
        return out

    def zero(self, field, level):
        check(self.L.mg3d32_zero(self._h, field, level))

    def sync(self):
        check(self.L.mg3d32_sync(self._h))

    def fill_boundary(self, field, level):
        check(self.L.mg3d32_fill_boundary(self._h, field, level))

    def smooth(self, level, iters):
        check(self.L.mg3d32_smooth(self._h, level, iters))

    def residual(self, level, store=True, want_norm=True):
        n = C.c_double(0)
        check(self.L.mg3d32_residual(self._h, level, 1 if store else 0, C.byref(n) if want_norm else None))
        return n.value

    def restrict(self, level):
        check(self.L.mg3d32_restrict(self._h, level))

    def prolong(self, level):
        check(self.L.mg3d32_prolong(self._h, level))

    def coarse_solve(self):
        check(self.L.mg3d32_coarse_solve(self._h))

    def setup_test_problem(self, fmg=False):
        """test_mg_3d.c:11-29: boundary values on the faces of the finest u and d; with fmg=True on the faces of d
        on every level (the F-cycle start of mg_dirichlet_analytic.c:771-806 reads them), then that start."""
        top = self.num_levels - 1
        for l in range(self.num_levels):  # a clean hierarchy, as after the reference's calloc (mg_3d.h:44)
            for f in (MG3D_U, MG3D_D, MG3D_R):
                self.zero(f, l)
        if fmg:
            for l in range(self.num_levels):
                self.fill_boundary(MG3D_D, l)
            check(self.L.mg3d32_fmg_initialize(self._h))
        else:
            self.fill_boundary(MG3D_U, top)
            self.fill_boundary(MG3D_D, top)

    def vcycles(self, count):
        norms = np.zeros(count)
        check(self.L.mg3d32_vcycles(self._h, count, P(norms)))
        return norms


class DistSolver32:
    """`Solver32` on i-slabs: rank `rank` of `nranks` (one process per GPU, RCCL), or -- unique_id=None -- all ranks
    virtual in this process on one GPU (loopback transport)."""

    def __init__(self, coarse_pts, num_levels, smooth_iters, omega=6.0 / 7.0, rank=0, nranks=1, unique_id=None, device=0,
                 grid_length=1.0):
        self.L = lib()
        self._h = C.c_void_p()
        uid = None if unique_id is None else C.c_char_p(bytes(unique_id))
        check(self.L.mg3d32_dist_create(coarse_pts, num_levels, smooth_iters, omega, grid_length, rank, nranks, uid,
                                        device, C.byref(self._h)))
        self.c, self.num_levels, self.nu, self.rank, self.nranks = coarse_pts, num_levels, smooth_iters, rank, nranks
        self.N = (coarse_pts - 1) * (1 << (num_levels - 1)) + 1
        self.first_level = self.L.mg3d32_dist_first_level(self._h)
        self.halo = self.L.mg3d32_dist_halo(self._h)

    def close(self):
        if self._h:
            check(self.L.mg3d32_dist_destroy(self._h))
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def level_n(self, level):
        return (self.c - 1) * (1 << level) + 1

    def comm_info(self):
        n, dev = C.c_int(0), C.c_int(0)
        check(self.L.mg3d32_dist_comm_info(self._h, C.byref(n), C.byref(dev)))
        return n.value, dev.value

    def upload(self, field, level, host_full):
        host_full = np.ascontiguousarray(host_full, dtype=np.float32).reshape(-1)
        assert host_full.size == self.level_n(level) ** 3
        check(self.L.mg3d32_dist_upload(self._h, field, level, PF(host_full)))

    def download(self, field, level, out=None):
        out = np.zeros(self.level_n(level) ** 3, dtype=np.float32) if out is None else out
        check(self.L.mg3d32_dist_download(self._h, field, level, PF(out)))
        return out

    def zero(self, field, level):
        check(self.L.mg3d32_dist_zero(self._h, field, level))

    def fill_boundary(self, field, level):
        check(self.L.mg3d32_dist_fill_boundary(self._h, field, level))

    def setup_test_problem(self, fmg=False):
        """As Solver32.setup_test_problem, every rank on its slab."""
        top = self.num_levels - 1
        for l in range(self.num_levels):
            for f in (MG3D_U, MG3D_D, MG3D_R):
                self.zero(f, l)
        if fmg:
            for l in range(self.num_levels):
                self.fill_boundary(MG3D_D, l)
            check(self.L.mg3d32_dist_fmg_initialize(self._h))
        else:
            self.fill_boundary(MG3D_U, top)
            self.fill_boundary(MG3D_D, top)

    def vcycles(self, count):
        norms = np.zeros(count)
        check(self.L.mg3d32_dist_vcycles(self._h, count, P(norms)))
        return norms

    def sync(self):
        check(self.L.mg3d32_dist_sync(self._h))
