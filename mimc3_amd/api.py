"""Host-side mirror of the reference's entry points for the hot path, over the C ABI
(include/mimc3_hip.h -> csrc/libmimc3_hip.so).

Names and argument meaning follow the reference (MIMC_module.h:41-58):
    get_uv_pivot, matching_ncc_dlc_2, get_ruv_neighbor, get_dpf_pseudosmoothing
with the ragged ``GMA_int32 **uv_pivot`` flattened to CSR ``(piv_off, piv_uv)`` and the ragged
``GMA_float **mvn_dp`` padded to ``[N][Kmax][5]`` + ``nclus[N]``.

Importing this module loads the HIP library and raises if it is missing: there is no CPU fallback
(the CPU restatement lives in oracle/ and is test infrastructure only).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MIMC3_HIP_LIB") or os.path.join(_HERE, "csrc", "libmimc3_hip.so")   # (override: A/B builds in tools/)

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} not built. Run `make -C mimc3_amd/csrc` (or python -c 'import __graft_entry__ as g; g.build()'). "
        "mimc3_amd has no CPU fallback.")
_lib = C.CDLL(LIB_PATH)

_f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
_f64p = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
_i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_i64p = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")
_vp = C.c_void_p

# every symbol include/mimc3_hip.h declares (checked by tests/test_capi_symbols.py)
_lib.mimc3_last_error.restype = C.c_char_p
_lib.mimc3_version.restype = C.c_char_p
_lib.mimc3_ctx_create.argtypes = [C.c_int, C.POINTER(_vp)]
_lib.mimc3_ctx_destroy.argtypes = [_vp]
_lib.mimc3_ctx_destroy.restype = None
_lib.mimc3_ctx_set_images.argtypes = [_vp, _f32p, _f32p, C.c_int32, C.c_int32]
_lib.mimc3_ctx_set_images_dev.argtypes = [_vp, _vp, _vp, C.c_int32, C.c_int32]
_lib.mimc3_ctx_set_images_u8.argtypes = [_vp, _vp, _vp, C.c_int32, C.c_int32]
_lib.mimc3_ctx_set_images_u16.argtypes = [_vp, _vp, _vp, C.c_int32, C.c_int32]
_lib.mimc3_host_alloc.argtypes = [C.c_size_t]
_lib.mimc3_host_alloc.restype = _vp
_lib.mimc3_host_free.argtypes = [_vp]
_lib.mimc3_host_free.restype = None
_lib.mimc3_get_uv_pivot.argtypes = [_f64p, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32, C.c_int32,
                                    C.c_int32, _i64p, _vp, C.c_int64, C.POINTER(C.c_int64)]
_lib.mimc3_match_ncc_dlc.argtypes = [_vp, _f64p, C.c_int32, _i32p, _i32p, _i64p, C.c_int32, C.c_int32, _f32p]
_lib.mimc3_match_ncc_dlc_dev.argtypes = [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, C.c_int32, C.c_int32,
                                         C.c_int32, C.c_int32, C.c_int32, _vp, _vp]
_lib.mimc3_match_ncc_full.argtypes = [_vp, _f64p, C.c_int32, _i32p, _vp, C.c_int32, C.c_int32, C.c_int32, _f32p]
_lib.mimc3_match_ncc_full_dev.argtypes = [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp]
_lib.mimc3_match_ncc_full_multi.argtypes = [_vp, _f64p, C.c_int32, _i32p, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _f32p, _f32p]
_lib.mimc3_match_ncc_full_multi_dev.argtypes = [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                _vp, _vp, _vp]
_lib.mimc3_match_ncc_full_planes.argtypes = [_vp, _f64p, C.c_int32, _i32p, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _f32p, _vp]
_lib.mimc3_match_ncc_full_planes_dev.argtypes = [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                 _vp, _vp, _vp]
_lib.mimc3_match_ncc_full_dn.argtypes = [_vp, _f64p, C.c_int32, _i32p, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _f32p, _vp]
_lib.mimc3_match_ncc_full_any.argtypes = [_vp, _f64p, C.c_int32, _i32p, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _f32p,
                                          _vp, _vp]
_lib.mimc3_match_ncc_full_any_dev.argtypes = [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                              C.c_int32, _vp, _vp, _vp, _vp]
_lib.mimc3_match_ncc_full_chip.argtypes = [_vp, _f64p, C.c_int32, _i32p, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _f32p,
                                           _vp, _vp]
_lib.mimc3_match_ncc_full_chip_dev.argtypes = [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                               C.c_int32, _vp, _vp, _vp, _vp]
_lib.mimc3_match_ncc_full_chip_class.argtypes = _lib.mimc3_match_ncc_full_chip.argtypes
_lib.mimc3_match_ncc_full_chip_class_dev.argtypes = _lib.mimc3_match_ncc_full_chip_dev.argtypes
_lib.mimc3_full_chip_class_layout.argtypes = [C.c_int32, _vp]
_lib.mimc3_match_ncc_full_chip_planes.argtypes = _lib.mimc3_match_ncc_full_chip.argtypes
_lib.mimc3_match_ncc_full_chip_planes_dev.argtypes = _lib.mimc3_match_ncc_full_chip_dev.argtypes
_lib.mimc3_full_chip_planes_layout.argtypes = [C.c_int32, _vp]
_lib.mimc3_full_chip_max_ocw.argtypes = []
_lib.mimc3_full_chip_band_rows.argtypes = [C.c_int32, C.c_int32]
_lib.mimc3_match_ncc_full_surf.argtypes = [_vp, _f64p, C.c_int32, _i32p, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _f32p, _vp, _vp]
_lib.mimc3_match_ncc_full_surf_dev.argtypes = [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                               _vp, _vp, _vp, _vp]
_lib.mimc3_wide_max_radius.argtypes = [C.c_int32]
_lib.mimc3_wide_lds_bytes.argtypes = [C.c_int32, C.c_int32]
_lib.mimc3_match_ncc_wide.argtypes = [_vp, _f64p, C.c_int32, _i32p, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _f32p, _vp, _vp]
_lib.mimc3_match_ncc_wide_dev.argtypes = [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                          _vp, _vp, _vp, _vp]
_lib.mimc3_wide_class_max_radius.argtypes = [C.c_int32]
_lib.mimc3_wide_class_layout.argtypes = [C.c_int32, C.c_int32, _vp]
_lib.mimc3_match_ncc_wide_class.argtypes = _lib.mimc3_match_ncc_full_chip.argtypes
_lib.mimc3_match_ncc_wide_class_dev.argtypes = _lib.mimc3_match_ncc_full_chip_dev.argtypes
_lib.mimc3_wide_planes_max_radius.argtypes = [C.c_int32]
_lib.mimc3_wide_planes_layout.argtypes = [C.c_int32, C.c_int32, _vp]
_lib.mimc3_match_ncc_wide_planes.argtypes = _lib.mimc3_match_ncc_full_chip.argtypes
_lib.mimc3_match_ncc_wide_planes_dev.argtypes = _lib.mimc3_match_ncc_full_chip_dev.argtypes
_lib.mimc3_wide_chip_max_radius.argtypes = [C.c_int32]
_lib.mimc3_wide_chip_layout.argtypes = [C.c_int32, C.c_int32, _vp]
_lib.mimc3_wide_chip_path.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32]
_lib.mimc3_match_ncc_wide_chip.argtypes = _lib.mimc3_match_ncc_full_chip.argtypes
_lib.mimc3_match_ncc_wide_chip_dev.argtypes = _lib.mimc3_match_ncc_full_chip_dev.argtypes
_lib.mimc3_match_ncc_full_dn_dev.argtypes = [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                             _vp, _vp, _vp]
_lib.mimc3_match_ncc_full_fb.argtypes = [_vp, _f64p, C.c_int32, _i32p, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _f32p, _vp, _vp]
_lib.mimc3_match_ncc_full_fb_dev.argtypes = [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                             _vp, _vp, _vp, _vp]
_lib.mimc3_match_ncc_wide_fb.argtypes = [_vp, _f64p, C.c_int32, _i32p, _vp, C.c_int32, C.c_int32, C.c_int32, _f32p, _vp, _vp]
_lib.mimc3_match_ncc_wide_fb_dev.argtypes = [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp,
                                             _vp]
_lib.mimc3_stack_begin.argtypes = [_vp, C.c_int32, C.c_int32, _vp]
_lib.mimc3_stack_begin_wide.argtypes = [_vp, C.c_int32, C.c_int32, _vp]
_lib.mimc3_stack_chunk.argtypes = [C.c_int32]
_lib.mimc3_stack_chunk.restype = C.c_int32
_lib.mimc3_stack_add.argtypes = [_vp, _f64p, C.c_int32, _i32p, C.c_int32, C.c_int32]
_lib.mimc3_stack_add_dev.argtypes = [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp]
_lib.mimc3_stack_add_class.argtypes = [_vp, _f64p, C.c_int32, _i32p, C.c_int32, C.c_int32]
_lib.mimc3_stack_add_class_dev.argtypes = [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp]
_lib.mimc3_stack_add_fused.argtypes = [_vp, _f64p, C.c_int32, _i32p, C.c_int32, C.c_int32]
_lib.mimc3_stack_add_fused_dev.argtypes = [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp]
_lib.mimc3_stack_fused_max_radius.argtypes = [_vp, C.c_int32]
_lib.mimc3_stack_fused_max_radius.restype = C.c_int32
_lib.mimc3_stack_add_surfaces.argtypes = [_vp, _f32p, _vp, C.c_int32]
_lib.mimc3_stack_add_surfaces_dev.argtypes = [_vp, _vp, _vp, C.c_int32, _vp]
_lib.mimc3_stack_finish.argtypes = [_vp, C.c_int32, C.c_int32, _f32p, _vp, _vp, _vp]
_lib.mimc3_stack_finish_dev.argtypes = [_vp, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp]
_lib.mimc3_stack_info.argtypes = [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
_lib.mimc3_stack_layer_radius.argtypes = [C.c_int32, C.c_double]
_lib.mimc3_stack_layer_radius.restype = C.c_int32
_lib.mimc3_stack_layer_shift.argtypes = [_vp, C.c_double, _i32p]
_lib.mimc3_stack_weighted.argtypes = [_vp]
_lib.mimc3_stack_add_scaled.argtypes = [_vp, _f64p, C.c_int32, _i32p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double]
_lib.mimc3_stack_add_scaled_dev.argtypes = [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double,
                                            C.c_double, _vp]
_lib.mimc3_stack_add_scaled_fused.argtypes = [_vp, _f64p, C.c_int32, _i32p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double]
_lib.mimc3_stack_add_scaled_fused_dev.argtypes = [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double,
                                                  C.c_double, _vp]
_lib.mimc3_stack_add_surfaces_scaled.argtypes = [_vp, _f32p, _vp, C.c_int32, C.c_int32, C.c_double, C.c_double]
_lib.mimc3_stack_add_surfaces_scaled_dev.argtypes = [_vp, _vp, _vp, C.c_int32, C.c_int32, C.c_double, C.c_double, _vp]
_lib.mimc3_match_ncc_pyramid.argtypes = [_vp, _f64p, C.c_int32, _i32p, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _f32p, _i32p]
_lib.mimc3_match_ncc_pyramid_dev.argtypes = [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                             _vp, _vp, _vp]
_lib.mimc3_match_ncc_pyramid_dn.argtypes = [_vp, _f64p, C.c_int32, _i32p, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _f32p, _vp,
                                            _i32p]
_lib.mimc3_match_ncc_pyramid_dn_dev.argtypes = [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                C.c_int32, _vp, _vp, _vp, _vp]
_lib.mimc3_match_ncc_pyramid_any.argtypes = [_vp, _f64p, C.c_int32, _i32p, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                             _f32p, _vp, _i32p]
_lib.mimc3_match_ncc_pyramid_any_dev.argtypes = [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                 C.c_int32, C.c_int32, _vp, _vp, _vp, _vp]
_lib.mimc3_match_ncc_pyramid_chip.argtypes = _lib.mimc3_match_ncc_pyramid_any.argtypes
_lib.mimc3_match_ncc_pyramid_chip_dev.argtypes = _lib.mimc3_match_ncc_pyramid_any_dev.argtypes
_lib.mimc3_pyramid_chip_path.argtypes = [C.c_int32, C.c_int32, C.c_int32]
_lib.mimc3_ctx_get_pyramid_level.argtypes = [_vp, C.c_int32, _f32p, _f32p]
_lib.mimc3_ctx_get_pyramid_level_any.argtypes = [_vp, C.c_int32, _f32p, _f32p]
_lib.mimc3_prior_shift.argtypes = [_f64p, C.c_int32, C.c_float, C.c_float, _i32p]
_lib.mimc3_pivot_corridors.argtypes = [_f64p, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, _vp]
_lib.mimc3_get_uv_pivot_dev.argtypes = [_vp, _vp, _vp, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_int64, C.POINTER(C.c_int64), _i32p, _vp]
_lib.mimc3_match_ncc_dlc_geo.argtypes = [_vp, _f64p, C.c_int32, _i32p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32, C.c_int32, _f32p]
_lib.mimc3_match_ncc_dlc_cor.argtypes = [_vp, _f64p, _vp, C.c_int32, _i32p, C.c_int32, C.c_int32, _f32p]
_lib.mimc3_qm_launches_per_sweep.restype = C.c_int32
_lib.mimc3_pivot_extent.argtypes = [_i32p, _i64p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                    C.POINTER(C.c_int32)]
_lib.mimc3_get_ruv_neighbor.argtypes = [_f64p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, _i32p, C.c_int32,
                                        C.POINTER(C.c_int32)]
_lib.mimc3_qm_pseudosmooth.argtypes = [_vp, C.c_int32, C.c_int32, _i32p, _f32p, _f32p, _i32p, C.c_int32, _f32p,
                                       C.c_int32, _i32p, _f64p, C.c_int32, C.POINTER(C.c_int32)]
_lib.mimc3_qm_workspace_bytes.argtypes = [C.c_int32, C.c_int32]
_lib.mimc3_qm_workspace_bytes.restype = C.c_int64
_lib.mimc3_qm_pseudosmooth_dev.argtypes = [_vp, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, C.c_int32, _vp, C.c_int32, _vp,
                                           _vp, C.c_int32, _vp, _vp, _vp]
_lib.mimc3_cluster_candidates.argtypes = [_vp, _f32p, C.c_int32, C.c_int32, C.c_int32, _f32p, _i32p, C.POINTER(C.c_int32)]
_lib.mimc3_cluster_candidates_dev.argtypes = [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp]
_lib.mimc3_get_dpf0.argtypes = [_vp, _f32p, _i32p, C.c_int32, C.c_int32, C.c_float, _i32p]
_lib.mimc3_get_dpf0_dev.argtypes = [_vp, _vp, _vp, C.c_int32, C.c_int32, C.c_float, _vp, _vp]
_lib.mimc3_get_dpf1.argtypes = [_vp, C.c_int32, C.c_int32, _i32p, _f32p, _f32p, _i32p, C.c_int32, _f32p, C.c_int32, _i32p,
                                _f64p, C.c_float, C.c_float, C.POINTER(C.c_int32)]
_lib.mimc3_dpf1_workspace_bytes.argtypes = [C.c_int32]
_lib.mimc3_dpf1_workspace_bytes.restype = C.c_int64
_lib.mimc3_get_dpf1_dev.argtypes = [_vp, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, C.c_int32, _vp, C.c_int32, _vp, _vp,
                                    C.c_float, C.c_float, _vp, C.POINTER(C.c_int32), _vp]
_lib.mimc3_float_conv2.argtypes = [_vp, _f32p, C.c_int32, C.c_int32, _f32p, C.c_int32, C.c_int32, _f32p]
_lib.mimc3_float_conv2_dev.argtypes = [_vp, _vp, C.c_int32, C.c_int32, _f32p, C.c_int32, C.c_int32, _vp, _vp, _vp]
_lib.mimc3_ctx_filter_images.argtypes = [_vp, _vp, C.c_int32, C.c_int32]
_lib.mimc3_ctx_get_images.argtypes = [_vp, _vp, _vp]


class CpParams(C.Structure):
    """mimc3_cp_params (include/mimc3_hip.h): the reference's globals that get_offset_image reads."""
    _fields_ = [("vec_ocw", C.c_int32 * 4), ("aw_cre", C.c_float), ("num_cp_max", C.c_int32), ("num_cp_min", C.c_int32),
                ("ratio_cp", C.c_float), ("thres_spd_cp", C.c_float), ("kernel", C.c_void_p * 3), ("kdim", (C.c_int32 * 2) * 3),
                ("seed", C.c_int64)]


_lib.mimc3_get_offset_image_multi.argtypes = [C.POINTER(_vp), C.c_int32, _f64p, C.c_int32, C.POINTER(CpParams), _i32p,
                                              np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS"), C.POINTER(C.c_int32), _i32p, _f32p]
_lib.mimc3_get_offset_image.argtypes = [_vp, _f64p, C.c_int32, C.POINTER(CpParams), _i32p,
                                        np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS"), C.POINTER(C.c_int32), _i32p, _f32p]


class VmapParams(C.Structure):
    """mimc3_vmap_params: the reference's `param_mimc2` + kernels (defaults = MIMC_main.c:134-194)."""
    _fields_ = [("vec_ocw", C.c_int32 * 4), ("aw_cre", C.c_float), ("aw_sf", C.c_float), ("radius_neighbor_dpf1", C.c_float),
                ("radius_neighbor_ps", C.c_float), ("num_cp_max", C.c_int32), ("num_cp_min", C.c_int32), ("ratio_cp", C.c_float),
                ("thres_spd_cp", C.c_float), ("kernel", C.c_void_p * 3), ("kdim", (C.c_int32 * 2) * 3), ("cp_seed", C.c_int64),
                ("qm_max_sweeps", C.c_int32)]


class VmapResult(C.Structure):
    _fields_ = [("dimx", C.c_int32), ("dimy", C.c_int32), ("mpp", C.c_float), ("spacing_grid", C.c_float),
                ("meter_per_spacing", C.c_float), ("cp_status", C.c_int32), ("offset_cp", C.c_int32 * 2), ("cp_subint", C.c_float * 2)]


CLI_KERNELS = (np.array([[-1, 0, 1]], np.float32), np.array([[-1], [0], [1]], np.float32),
               np.array([[-1 / 8] * 3, [-1 / 8, 1, -1 / 8], [-1 / 8] * 3], np.float32))     # MIMC_main.c:176-194

_lib.mimc3_postprocess.argtypes = [_vp, _f32p, C.c_int32, _f64p, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float,
                                   C.c_float, C.c_int32, _f32p]
_lib.mimc3_vmap.argtypes = [_vp, _f64p, C.c_int32, C.c_float, C.POINTER(VmapParams), _f32p, _f32p, _f32p, _f32p, _f32p,
                            np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS"), C.POINTER(VmapResult)]
_lib.mimc3_vmap_passes.argtypes = [_vp, _f64p, C.c_int32, C.c_float, C.POINTER(VmapParams), C.c_int32, C.c_int32, _vp,
                                   np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS"), C.POINTER(VmapResult)]
_lib.mimc3_vmap_finish.argtypes = [_vp, _f64p, C.c_int32, C.c_float, C.POINTER(VmapParams), _vp, _f32p, _f32p, _f32p, _f32p, _f32p,
                                   C.POINTER(VmapResult)]
_lib.mimc3_vmap_geometry.argtypes = [_f64p, C.c_int32, C.POINTER(VmapResult)]
_lib.mimc3_vmap_cp.argtypes = [_vp, _f64p, C.c_int32, C.c_float, C.POINTER(VmapParams), np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS"),
                               C.POINTER(VmapResult)]
_lib.mimc3_vmap_passes_points.argtypes = [_vp, _f64p, C.c_int32, C.c_float, C.POINTER(VmapParams), C.POINTER(VmapResult), _vp, C.c_int64]
_lib.mimc3_ctx_set_path.argtypes = [_vp, C.c_int32]
_lib.mimc3_ctx_last_path.argtypes = [_vp]
_lib.mimc3_ctx_enable_timing.argtypes = [_vp, C.c_int32]
_lib.mimc3_ctx_last_kernel_ms.argtypes = [_vp, C.POINTER(C.c_float)]


_lib.mimc3_point_cost.argtypes = [_i64p, C.c_int32, C.c_int32, _f64p]
_lib.mimc3_partition_points.argtypes = [_f64p, C.c_int32, C.c_int32, C.c_int32, _i32p, _i32p, C.POINTER(C.c_double)]
_lib.mimc3_mgpu_create.argtypes = [_i32p, C.c_int32, C.POINTER(_vp)]
_lib.mimc3_mgpu_create_ex.argtypes = [_i32p, C.c_int32, C.c_char_p, C.c_uint32, C.POINTER(_vp)]
_lib.mimc3_mgpu_destroy.argtypes = [_vp]
_lib.mimc3_mgpu_destroy.restype = None
_lib.mimc3_mgpu_ndev.argtypes = [_vp]
_lib.mimc3_mgpu_ctx.argtypes = [_vp, C.c_int32]
_lib.mimc3_mgpu_ctx.restype = _vp
_lib.mimc3_mgpu_last_imbalance.argtypes = [_vp]
_lib.mimc3_mgpu_last_imbalance.restype = C.c_double
_lib.mimc3_mgpu_set_images.argtypes = [_vp, _f32p, _f32p, C.c_int32, C.c_int32]
_lib.mimc3_mgpu_set_images_u8.argtypes = [_vp, _vp, _vp, C.c_int32, C.c_int32]
_lib.mimc3_mgpu_set_images_u16.argtypes = [_vp, _vp, _vp, C.c_int32, C.c_int32]
_lib.mimc3_mgpu_match_ncc_dlc.argtypes = [_vp, _f64p, C.c_int32, _i32p, _i32p, _i64p, C.c_int32, C.c_int32, _f32p]
_lib.mimc3_mgpu_vmap.argtypes = [_vp, _f64p, C.c_int32, C.c_float, C.POINTER(VmapParams), _f32p, _f32p, _f32p, _f32p, _f32p,
                                 np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS"), C.POINTER(VmapResult)]
_lib.mimc3_ctx_device.argtypes = [_vp]
_lib.mimc3_ctx_workspace.argtypes = [_vp, C.c_int32, C.c_size_t, C.POINTER(_vp)]


class Mimc3Error(RuntimeError):
    def __init__(self, code, where):
        self.code = code
        msg = _lib.mimc3_last_error().decode(errors="replace")
        super().__init__(f"{where}: rc={code}: {msg}")


def _check(rc, where):
    if rc != 0:
        raise Mimc3Error(rc, where)


def version():
    return _lib.mimc3_version().decode()


def _ptr(a):
    return None if a is None else a.ctypes.data


def _search_arrays(what, xyuvav, shift, npeaks=0, radius=0, surface=False, fb=False):
    """What a host wrapper of the exhaustive-search family hands to the library -> (xy float64[n][6], n, out float32[n][8], cand
    float32[npeaks][n][3] or None when npeaks <= 0, surf float32[n][(2 radius + 1)^2] or None, fb float32[1 + npeaks][n][4] or None,
    shift int32[n][2] or None -- checked: ValueError on another shape)."""
    xy = np.ascontiguousarray(xyuvav, np.float64)
    n = xy.shape[0]
    npeaks = int(npeaks)
    out = np.empty((n, 8), np.float32)
    cand = np.empty((npeaks, n, 3), np.float32) if npeaks > 0 else None
    surf = np.empty((n, (2 * int(radius) + 1) ** 2), np.float32) if surface else None
    rows = np.empty((1 + max(npeaks, 0), n, 4), np.float32) if fb else None
    sh = None
    if shift is not None:
        sh = np.ascontiguousarray(shift, np.int32)
        if sh.shape != (n, 2):
            raise ValueError(f"{what}: shift must be int32[{n}][2], got {sh.shape}")
    return xy, n, out, cand, surf, rows, sh


def wide_max_radius(ocw):
    """The largest radius match_ncc_wide takes at this chip size (mimc3_wide_max_radius); 0 for an ocw it does not take."""
    return int(_lib.mimc3_wide_max_radius(int(ocw)))


def pyramid_chip_path(pair_class, ocw, mode):
    """The last_path of match_ncc_pyramid_chip for a pair class (0 8-bit, 1 scaled-integer, 2 integral f32, 3 any other), a chip
    half-width and a mode (mimc3_pyramid_chip_path; no device): 6 / 12, 13, 8 / 11, 9 / 11 -- 0 for anything outside the table."""
    return int(_lib.mimc3_pyramid_chip_path(int(pair_class), int(ocw), int(mode)))


def full_chip_max_ocw():
    """The largest chip half-width match_ncc_full_chip takes (mimc3_full_chip_max_ocw): 80."""
    return int(_lib.mimc3_full_chip_max_ocw())


def full_chip_class_layout(ocw):
    """The layout of match_ncc_full_chip_class's matrix-core kernel at this chip half-width (mimc3_full_chip_class_layout) -> (K chunks of
    64 window columns per chip row, 16-row tiles of the box sums, K chunks of the box sums, dynamic LDS bytes); None outside
    1 <= ocw <= full_chip_max_ocw()."""
    out = (C.c_int32 * 4)()
    return tuple(int(v) for v in out) if _lib.mimc3_full_chip_class_layout(int(ocw), out) else None


def full_chip_planes_layout(ocw):
    """The layout of match_ncc_full_chip_planes's matrix-core kernel on the u16 planes at this chip half-width
    (mimc3_full_chip_planes_layout) -> (K chunks of 64 window columns per chip row, 16-row tiles of the box sums, K chunks of the box sums,
    dynamic LDS bytes); None outside 1 <= ocw <= full_chip_max_ocw()."""
    out = (C.c_int32 * 4)()
    return tuple(int(v) for v in out) if _lib.mimc3_full_chip_planes_layout(int(ocw), out) else None


def full_chip_band_rows(ocw, radius):
    """The chip rows of one band of match_ncc_full_chip's kernel (mimc3_full_chip_band_rows): 2 ocw + 1 where the whole chip is one
    band; 0 outside 1 <= ocw <= full_chip_max_ocw(), 1 <= radius <= 15."""
    return int(_lib.mimc3_full_chip_band_rows(int(ocw), int(radius)))


def wide_class_max_radius(ocw):
    """The largest radius match_ncc_wide_class takes at this chip half-width (mimc3_wide_class_max_radius): 47 for 1 <= ocw <=
    full_chip_max_ocw(), else 0."""
    return int(_lib.mimc3_wide_class_max_radius(int(ocw)))


def wide_class_layout(ocw, radius):
    """The layout of match_ncc_wide_class's matrix-core kernel (mimc3_wide_class_layout) -> (K chunks of 64 window columns per chip row,
    32 x 32 cell tiles per axis, threads per workgroup, dynamic LDS bytes); None outside 1 <= ocw <= full_chip_max_ocw(),
    16 <= radius <= 47."""
    out = (C.c_int32 * 4)()
    return tuple(int(v) for v in out) if _lib.mimc3_wide_class_layout(int(ocw), int(radius), out) else None


def wide_planes_max_radius(ocw):
    """The largest radius match_ncc_wide_planes's matrix-core kernel on the u16 planes takes at this chip half-width
    (mimc3_wide_planes_max_radius): the largest radius <= 47 whose layout fits the LDS of a CU -- 47 for ocw 1..68, falling to 27 at ocw
    80; 0 outside 1 <= ocw <= full_chip_max_ocw()."""
    return int(_lib.mimc3_wide_planes_max_radius(int(ocw)))


def wide_planes_layout(ocw, radius):
    """The layout of match_ncc_wide_planes's matrix-core kernel (mimc3_wide_planes_layout) -> (K chunks of 64 window columns per chip row,
    32 x 32 cell tiles per axis, threads per workgroup, dynamic LDS bytes); None outside 1 <= ocw <= full_chip_max_ocw(),
    16 <= radius <= wide_planes_max_radius(ocw)."""
    out = (C.c_int32 * 4)()
    return tuple(int(v) for v in out) if _lib.mimc3_wide_planes_layout(int(ocw), int(radius), out) else None


def wide_chip_max_radius(ocw):
    """The largest radius match_ncc_wide_chip takes at this chip half-width (mimc3_wide_chip_max_radius): 47 for 1 <= ocw <=
    full_chip_max_ocw(), else 0."""
    return int(_lib.mimc3_wide_chip_max_radius(int(ocw)))


def wide_chip_layout(ocw, radius):
    """The layout of match_ncc_wide_chip's run-time-ocw wide float kernel (mimc3_wide_chip_layout) -> (32 x 32 cell tiles per axis, chip
    rows per band, bands, workgroups per CU the LDS allows, dynamic LDS bytes); None outside 1 <= ocw <= full_chip_max_ocw(),
    16 <= radius <= 47."""
    out = (C.c_int32 * 5)()
    return tuple(int(v) for v in out) if _lib.mimc3_wide_chip_layout(int(ocw), int(radius), out) else None


def wide_chip_path(pair_class, ocw, radius, mode):
    """The last_path of match_ncc_wide_chip for a pair class (0 8-bit, 1 scaled-integer, 2 integral f32, 3 any other), a chip half-width,
    a radius and a mode (mimc3_wide_chip_path; no device); -1 for anything outside the table."""
    return int(_lib.mimc3_wide_chip_path(int(pair_class), int(ocw), int(radius), int(mode)))


def wide_lds_bytes(ocw, radius):
    """The dynamic LDS (bytes) of the wide kernel's launch (mimc3_wide_lds_bytes); 0 outside 1 .. wide_max_radius(ocw)."""
    return int(_lib.mimc3_wide_lds_bytes(int(ocw), int(radius)))


# ---------------------------------------------------------------------------------------------
# host-side geometry (no GPU needed)
# ---------------------------------------------------------------------------------------------
def get_uv_pivot(xyuvav, dt, mpp, ocw, H, W, aw_sf=1.8, aw_cre=10.0):
    """get_uv_pivot (MIMC_module.c:543-602) -> CSR (piv_off int64[N+1], piv_uv int32[P][2])."""
    xy = np.ascontiguousarray(xyuvav, np.float64)
    n = xy.shape[0]
    off = np.zeros(n + 1, np.int64)
    tot = C.c_int64(0)
    _check(_lib.mimc3_get_uv_pivot(xy, n, dt, mpp, aw_sf, aw_cre, ocw, H, W, off, None, 0, C.byref(tot)), "get_uv_pivot")
    uv = np.zeros((tot.value, 2), np.int32)
    _check(_lib.mimc3_get_uv_pivot(xy, n, dt, mpp, aw_sf, aw_cre, ocw, H, W, off, uv.ctypes.data_as(_vp), tot.value,
                                   C.byref(tot)), "get_uv_pivot")
    return off, uv


def get_uv_pivot_counts(xyuvav, dt, mpp, ocw, H, W, aw_sf=1.8, aw_cre=10.0):
    """The counting half of get_uv_pivot (MIMC_module.c:576-585): CSR offsets only (piv_off int64[N+1])."""
    xy = np.ascontiguousarray(xyuvav, np.float64)
    off = np.zeros(xy.shape[0] + 1, np.int64)
    tot = C.c_int64(0)
    _check(_lib.mimc3_get_uv_pivot(xy, xy.shape[0], dt, mpp, aw_sf, aw_cre, ocw, H, W, off, None, 0, C.byref(tot)), "get_uv_pivot")
    return off


CORRIDOR_BYTES = 24      # MIMC3_CORRIDOR_BYTES
STACK_CHUNK = 65536      # MIMC3_STACK_CHUNK: the points of one launch of Context.stack_add


def stack_chunk(radius):
    """The points of one accumulation launch of the stack at this radius (mimc3_stack_chunk): STACK_CHUNK up to 15, fewer beyond (57,832 at
    16, 6,978 at 47), 0 for a radius no stack takes."""
    return int(_lib.mimc3_stack_chunk(int(radius)))


def stack_layer_radius(radius, scale):
    """The smallest layer radius that serves every cell of a stack of this radius from a layer at `scale` (mimc3_stack_layer_radius):
    radius at scale 1, else floor(scale radius + 0.5) + 1; 0 for a radius outside 1..47 or a scale outside 1/64..64.  May exceed what a
    search takes (wide_max_radius(ocw)): pass a smaller radius then, and the stack's outer cells get no count from that layer."""
    return int(_lib.mimc3_stack_layer_radius(int(radius), float(scale)))


def prior_shift(xyuvav, dt, mpp):
    """The a-priori displacement in whole pixels, get_uv_pivot's sign convention -> int32[N][2]:
    (floor(vx dt / 365 / mpp + 0.5), floor(-vy dt / 365 / mpp + 0.5)) -- the search centres of match_ncc_full."""
    xy = np.ascontiguousarray(xyuvav, np.float64)
    out = np.empty((xy.shape[0], 2), np.int32)
    _check(_lib.mimc3_prior_shift(xy, xy.shape[0], dt, mpp, out), "prior_shift")
    return out


def pivot_corridors(xyuvav, dt, mpp, aw_sf=1.8, aw_cre=10.0):
    """the host half of get_uv_pivot (MIMC_module.c:559-573): [N] opaque 24-byte corridor records (uint8 [N][24])"""
    xy = np.ascontiguousarray(xyuvav, np.float64)
    cor = np.zeros((xy.shape[0], CORRIDOR_BYTES), np.uint8)
    _check(_lib.mimc3_pivot_corridors(xy, xy.shape[0], dt, mpp, aw_sf, aw_cre, cor.ctypes.data), "pivot_corridors")
    return cor


def qm_launches_per_sweep():
    return int(_lib.mimc3_qm_launches_per_sweep())


def pivot_extent(piv_off, piv_uv):
    mn, mu, mv = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    off = np.ascontiguousarray(piv_off, np.int64)
    _check(_lib.mimc3_pivot_extent(np.ascontiguousarray(piv_uv, np.int32), off, off.shape[0] - 1, C.byref(mn), C.byref(mu),
                                   C.byref(mv)), "pivot_extent")
    return mn.value, mu.value, mv.value


def get_ruv_neighbor(xyuvav, dimx, dimy, meter_per_spacing, radius, cap=4096):
    """get_ruv_neighbor (MIMC_module.c:1266-1327) -> int32[nn][2]."""
    xy = np.ascontiguousarray(xyuvav, np.float64)
    ruv = np.zeros((cap, 2), np.int32)
    nn = C.c_int32(0)
    _check(_lib.mimc3_get_ruv_neighbor(xy, xy.shape[0], dimx, dimy, meter_per_spacing, radius, ruv, cap, C.byref(nn)),
           "get_ruv_neighbor")
    return np.ascontiguousarray(ruv[:nn.value])


def pinned_empty(shape, dtype):
    """numpy array in pinned host memory (mimc3_host_alloc): host<->device copies of it need no staging.
    The block lives as long as ANY view of it: numpy keeps the ctypes buffer object as the base of the array and of every
    slice taken from it, and the block is freed by a finalizer on that buffer object (not on the first array)."""
    import weakref
    dt = np.dtype(dtype)
    count = int(np.prod(shape))
    nbytes = max(count * dt.itemsize, 1)
    p = _lib.mimc3_host_alloc(nbytes)
    if not p:
        raise MemoryError("mimc3_host_alloc failed")
    buf = (C.c_char * nbytes).from_address(p)
    weakref.finalize(buf, _lib.mimc3_host_free, p)
    a = np.frombuffer(buf, dtype=dt, count=count).reshape(shape)
    a.flags.writeable = True
    return a


def point_cost(piv_off, ocw, cost=None):
    """mimc3_point_cost: adds (4 + 6 npiv)(2 ocw + 1)^2 per point to `cost` (float64[N], created when None)."""
    off = np.ascontiguousarray(piv_off, np.int64)
    n = off.shape[0] - 1
    if cost is None:
        cost = np.zeros(n, np.float64)
    _check(_lib.mimc3_point_cost(off, n, ocw, cost), "point_cost")
    return cost


def partition_points(cost, world, block=1024):
    """mimc3_partition_points: cost-balanced block-cyclic shares.  Returns (order int32[N], start int32[world+1],
    imbalance = max load / mean load - 1); rank r owns grid points order[start[r]:start[r+1]]."""
    cost = np.ascontiguousarray(cost, np.float64)
    n = cost.shape[0]
    order = np.empty(n, np.int32)
    start = np.empty(world + 1, np.int32)
    imb = C.c_double(0)
    _check(_lib.mimc3_partition_points(cost, n, world, block, order, start, C.byref(imb)), "partition_points")
    return order, start, imb.value


class MultiGpu:
    """mimc3_mgpu: ONE process driving several GPUs (a host thread per device, RCCL communicator over them)."""

    def __init__(self, devices, comm_lib=None, repeat_devices=False):
        """comm_lib / repeat_devices: the test form (mimc3_mgpu_create_ex) -- a stand-in communicator library, N ranks on one device."""
        self._h = _vp()
        dv = np.ascontiguousarray(devices, np.int32)
        if comm_lib or repeat_devices:
            _check(_lib.mimc3_mgpu_create_ex(dv, dv.shape[0], comm_lib.encode() if comm_lib else None, 1 if repeat_devices else 0, C.byref(self._h)), "mgpu_create_ex")
        else:
            _check(_lib.mimc3_mgpu_create(dv, dv.shape[0], C.byref(self._h)), "mgpu_create")
        self.ndev = dv.shape[0]

    def close(self):
        if self._h:
            _lib.mimc3_mgpu_destroy(self._h)
            self._h = _vp()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_images(self, i0, i1):
        if i0.dtype in (np.uint8, np.uint16):
            i0 = np.ascontiguousarray(i0); i1 = np.ascontiguousarray(i1)
            fn = _lib.mimc3_mgpu_set_images_u8 if i0.dtype == np.uint8 else _lib.mimc3_mgpu_set_images_u16
            _check(fn(self._h, i0.ctypes.data, i1.ctypes.data, i0.shape[0], i0.shape[1]), "mgpu_set_images_raw")
        else:
            i0 = np.ascontiguousarray(i0, np.float32); i1 = np.ascontiguousarray(i1, np.float32)
            _check(_lib.mimc3_mgpu_set_images(self._h, i0, i1, i0.shape[0], i0.shape[1]), "mgpu_set_images")

    def matching_ncc_dlc_2(self, xyuvav, offset, piv_off, piv_uv, ocw, swap=False):
        xy = np.ascontiguousarray(xyuvav, np.float64)
        out = np.empty((xy.shape[0], 3), np.float32)
        _check(_lib.mimc3_mgpu_match_ncc_dlc(self._h, xy, xy.shape[0], np.ascontiguousarray(offset, np.int32),
                                             np.ascontiguousarray(piv_uv, np.int32), np.ascontiguousarray(piv_off, np.int64), ocw,
                                             1 if swap else 0, out), "mgpu_matching_ncc_dlc_2")
        return out

    def vmap(self, xyuvav, dt, **kw):
        xy = np.ascontiguousarray(xyuvav, np.float64)
        n = xy.shape[0]
        p, _keep = Context._vmap_params(**kw)
        planes = [np.empty(n, np.float32) for _ in range(5)]
        flag = np.zeros(n, np.uint8)
        r = VmapResult()
        _check(_lib.mimc3_mgpu_vmap(self._h, xy, n, dt, C.byref(p), *planes, flag, C.byref(r)), "mgpu_vmap")
        return Context._vmap_out(r, flag, planes)

    def last_imbalance(self):
        return float(_lib.mimc3_mgpu_last_imbalance(self._h))


# ---------------------------------------------------------------------------------------------
# device context
# ---------------------------------------------------------------------------------------------
class Context:
    """Owns a HIP stream and the resident image pair (mimc3_ctx)."""

    def __init__(self, device=0):
        self._h = _vp()
        _check(_lib.mimc3_ctx_create(device, C.byref(self._h)), "ctx_create")
        self.device = device
        self.H = self.W = 0
        self._keep = None

    def close(self):
        if self._h:
            _lib.mimc3_ctx_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- images -------------------------------------------------------------------------------
    def set_images(self, i0, i1):
        i0 = np.ascontiguousarray(i0, np.float32)
        i1 = np.ascontiguousarray(i1, np.float32)
        assert i0.shape == i1.shape and i0.ndim == 2
        self.H, self.W = i0.shape
        _check(_lib.mimc3_ctx_set_images(self._h, i0, i1, self.H, self.W), "ctx_set_images")

    def set_images_raw(self, i0, i1):
        """The pair as the TIFF holds it (uint8 or uint16 arrays): raw DN crosses PCIe, the widening to float32 of
        GMA_float_load_tiff (GMA.c:288-310) runs on the device.  Arrays from pinned_empty() are DMA'd without staging."""
        assert i0.shape == i1.shape and i0.ndim == 2 and i0.dtype == i1.dtype and i0.dtype in (np.uint8, np.uint16)
        i0 = np.ascontiguousarray(i0); i1 = np.ascontiguousarray(i1)
        self.H, self.W = i0.shape
        fn = _lib.mimc3_ctx_set_images_u8 if i0.dtype == np.uint8 else _lib.mimc3_ctx_set_images_u16
        _check(fn(self._h, i0.ctypes.data, i1.ctypes.data, self.H, self.W), "ctx_set_images_raw")

    def set_images_dev(self, d_i0, d_i1, H, W, keep=None):
        """d_i0/d_i1: integer device addresses (e.g. torch tensor.data_ptr()); keep = objects to hold."""
        self.H, self.W = H, W
        self._keep = keep
        _check(_lib.mimc3_ctx_set_images_dev(self._h, d_i0, d_i1, H, W), "ctx_set_images_dev")

    # -- matcher ------------------------------------------------------------------------------
    def matching_ncc_dlc_2(self, xyuvav, offset, piv_off, piv_uv, ocw, swap=False):
        """matching_ncc_dlc_2 (MIMC_module.c:805-842) on the resident pair -> float32[N][3].
        swap=True = the CLI's "swapped forward" pass (chip from i1, window from i0)."""
        xy = np.ascontiguousarray(xyuvav, np.float64)
        n = xy.shape[0]
        out = np.empty((n, 3), np.float32)
        _check(_lib.mimc3_match_ncc_dlc(self._h, xy, n, np.ascontiguousarray(offset, np.int32),
                                        np.ascontiguousarray(piv_uv, np.int32), np.ascontiguousarray(piv_off, np.int64),
                                        ocw, 1 if swap else 0, out), "matching_ncc_dlc_2")
        return out

    def matching_ncc_dlc_geo(self, xyuvav, offset, dt, mpp, ocw, swap=False, aw_sf=1.8, aw_cre=10.0, out=None):
        """get_uv_pivot + matching_ncc_dlc_2 in one call: corridors from the host (made chunk by chunk under the device's work), pivot
        lists made on the device.  swap=True = the swapped pass (images exchanged, pivots negated; the caller negates offset and
        (du, dv)).  `out` may be a pinned array (as for matching_ncc_dlc_cor)."""
        xy = np.ascontiguousarray(xyuvav, np.float64)
        if out is None:
            out = np.empty((xy.shape[0], 3), np.float32)
        _check(_lib.mimc3_match_ncc_dlc_geo(self._h, xy, xy.shape[0], np.ascontiguousarray(offset, np.int32), dt, mpp, aw_sf, aw_cre, ocw,
                                            1 if swap else 0, out), "matching_ncc_dlc_geo")
        return out

    def matching_ncc_dlc_cor(self, xyuvav, cor, offset, ocw, swap=False, out=None):
        """the same with the corridors given (pivot_corridors(): once per grid, whatever the chip size); `out` may be a pinned array"""
        xy = np.ascontiguousarray(xyuvav, np.float64)
        if out is None:
            out = np.empty((xy.shape[0], 3), np.float32)
        cor = np.ascontiguousarray(cor, np.uint8)
        _check(_lib.mimc3_match_ncc_dlc_cor(self._h, xy, cor.ctypes.data, xy.shape[0], np.ascontiguousarray(offset, np.int32), ocw, 1 if swap else 0, out),
               "matching_ncc_dlc_cor")
        return out

    def get_uv_pivot_dev(self, d_xyuvav, d_cor, n, ocw, d_piv_off, d_piv_uv=None, d_piv_uv_neg=None, cap=0, stream=0):
        """device half of get_uv_pivot on device buffers; returns (total, (max_npiv, max_abs_u, max_abs_v))"""
        total = C.c_int64(0)
        ext = np.zeros(3, np.int32)
        _check(_lib.mimc3_get_uv_pivot_dev(self._h, d_xyuvav, d_cor, n, ocw, d_piv_off, d_piv_uv, d_piv_uv_neg, cap, C.byref(total), ext, stream),
               "get_uv_pivot_dev")
        return total.value, (int(ext[0]), int(ext[1]), int(ext[2]))

    def matching_ncc_dlc_2_dev(self, d_xyuvav, n, offset, d_piv_uv, d_piv_off, extent, ocw, d_out, stream=0, swap=False):
        """Device-pointer variant (enqueue only). extent = pivot_extent(...) = (max_npiv, max|u|, max|v|)."""
        mn, mu, mv = extent
        _check(_lib.mimc3_match_ncc_dlc_dev(self._h, d_xyuvav, n, int(offset[0]), int(offset[1]), d_piv_uv, d_piv_off,
                                            mn, mu, mv, ocw, 1 if swap else 0, d_out, stream), "matching_ncc_dlc_2_dev")

    # -- exhaustive search ----------------------------------------------------------------------
    def match_ncc_full(self, xyuvav, offset, ocw, radius, shift=None, swap=False):
        """Exhaustive-search NCC offsets with peak quality (mimc3_match_ncc_full) on the resident 8-bit pair -> float32[N][8]:
        du, dv, ncc_peak (or the status -2 / -3 / -4), ncc_fit, snr, h_uu, h_uv, h_vv.  Every offset in [-radius, radius]^2
        around uv0 + offset + shift[i] (shift int32[N][2] or None)."""
        xy, n, out, cand, surf, fb, sh = _search_arrays("match_ncc_full", xyuvav, shift)
        _check(_lib.mimc3_match_ncc_full(self._h, xy, n, np.ascontiguousarray(offset, np.int32),
                                         _ptr(sh), ocw, radius, 1 if swap else 0, out), "match_ncc_full")
        return out

    def match_ncc_full_dev(self, d_xyuvav, n, offset, ocw, radius, d_out, d_shift=0, stream=0, swap=False):
        """Device-pointer variant (enqueue only): d_xyuvav [n][6] f64, d_shift [n][2] int32 or 0, d_out [n][8] f32."""
        _check(_lib.mimc3_match_ncc_full_dev(self._h, d_xyuvav, n, int(offset[0]), int(offset[1]), d_shift or None, ocw, radius,
                                             1 if swap else 0, d_out, stream), "match_ncc_full_dev")

    def match_ncc_full_multi(self, xyuvav, offset, ocw, radius, npeaks, shift=None, swap=False):
        """The exhaustive search with candidates (mimc3_match_ncc_full_multi) -> (float32[N][8] record, exactly match_ncc_full's,
        float32[npeaks][N][3] candidates): per point the best npeaks (1..8) local maxima of its correlation surface as (du, dv, ncc),
        by NCC descending, pass-major -- the dp that cluster_candidates / mimc2_postprocess read.  Slots without a peak are
        (NaN, NaN, -2), or (NaN, NaN, -3) at an invalid point."""
        xy, n, out, cand, surf, fb, sh = _search_arrays("match_ncc_full_multi", xyuvav, shift, npeaks=npeaks)
        _check(_lib.mimc3_match_ncc_full_multi(self._h, xy, n, np.ascontiguousarray(offset, np.int32),
                                               _ptr(sh), ocw, radius, int(npeaks), 1 if swap else 0, out,
                                               np.empty(1, np.float32) if cand is None else cand.reshape(-1)), "match_ncc_full_multi")
        return out, cand

    def match_ncc_full_multi_dev(self, d_xyuvav, n, offset, ocw, radius, npeaks, d_out, d_cand, d_shift=0, stream=0, swap=False):
        """Device-pointer variant (enqueue only): as match_ncc_full_dev, plus d_cand [npeaks][n][3] f32."""
        _check(_lib.mimc3_match_ncc_full_multi_dev(self._h, d_xyuvav, n, int(offset[0]), int(offset[1]), d_shift or None, ocw, radius,
                                                   npeaks, 1 if swap else 0, d_out, d_cand, stream), "match_ncc_full_multi_dev")

    def match_ncc_full_planes(self, xyuvav, offset, ocw, radius, npeaks=0, shift=None, swap=False):
        """The exhaustive search on the pair the context matches on (mimc3_match_ncc_full_planes): an 8-bit pair, or a scaled-integer
        one -- 12-bit DN, the pair after filter_images -> (float32[N][8] record as match_ncc_full, float32[npeaks][N][3] candidates
        as match_ncc_full_multi, or None when npeaks == 0)."""
        xy, n, out, cand, surf, fb, sh = _search_arrays("match_ncc_full_planes", xyuvav, shift, npeaks=npeaks)
        _check(_lib.mimc3_match_ncc_full_planes(self._h, xy, n, np.ascontiguousarray(offset, np.int32),
                                                _ptr(sh), ocw, radius, int(npeaks), 1 if swap else 0, out, _ptr(cand)), "match_ncc_full_planes")
        return out, cand

    def match_ncc_full_planes_dev(self, d_xyuvav, n, offset, ocw, radius, npeaks, d_out, d_cand=0, d_shift=0, stream=0, swap=False):
        """Device-pointer variant (enqueue only): as match_ncc_full_multi_dev; d_cand 0 with npeaks == 0."""
        _check(_lib.mimc3_match_ncc_full_planes_dev(self._h, d_xyuvav, n, int(offset[0]), int(offset[1]), d_shift or None, ocw, radius,
                                                    npeaks, 1 if swap else 0, d_out, d_cand or None, stream), "match_ncc_full_planes_dev")

    def match_ncc_full_dn(self, xyuvav, offset, ocw, radius, npeaks=0, shift=None, swap=False):
        """The exhaustive search on every pair the planes' matchers take (mimc3_match_ncc_full_dn): what match_ncc_full_planes takes,
        bit for bit, and an integral-f32 pair -- 16-bit DN, and what filter_images makes of it -> (float32[N][8] record,
        float32[npeaks][N][3] candidates, or None when npeaks == 0)."""
        xy, n, out, cand, surf, fb, sh = _search_arrays("match_ncc_full_dn", xyuvav, shift, npeaks=npeaks)
        _check(_lib.mimc3_match_ncc_full_dn(self._h, xy, n, np.ascontiguousarray(offset, np.int32),
                                            _ptr(sh), ocw, radius, int(npeaks), 1 if swap else 0, out, _ptr(cand)), "match_ncc_full_dn")
        return out, cand

    def match_ncc_full_dn_dev(self, d_xyuvav, n, offset, ocw, radius, npeaks, d_out, d_cand=0, d_shift=0, stream=0, swap=False):
        """Device-pointer variant (enqueue only): as match_ncc_full_planes_dev."""
        _check(_lib.mimc3_match_ncc_full_dn_dev(self._h, d_xyuvav, n, int(offset[0]), int(offset[1]), d_shift or None, ocw, radius,
                                                npeaks, 1 if swap else 0, d_out, d_cand or None, stream), "match_ncc_full_dn_dev")

    def match_ncc_full_any(self, xyuvav, offset, ocw, radius, npeaks=0, shift=None, swap=False, mode=0, surface=False):
        """The exhaustive search on any f32 pair (mimc3_match_ncc_full_any): mode 0 sends what match_ncc_full_dn takes where that sends it,
        bit for bit, and every other pair -- non-integral pixels, NaN or negative nulls -- through the float kernel ("f32g_full"); mode 1
        sends any pair through the float kernel -> (float32[N][8] record, float32[npeaks][N][3] candidates or None when npeaks == 0),
        and with surface=True (float kernel only) every point's NCC surface float32[N][(2 radius + 1)^2] in k order as a third item."""
        xy, n, out, cand, surf, fb, sh = _search_arrays("match_ncc_full_any", xyuvav, shift, npeaks=npeaks, radius=radius, surface=surface)
        _check(_lib.mimc3_match_ncc_full_any(self._h, xy, n, np.ascontiguousarray(offset, np.int32), _ptr(sh), ocw, radius, int(npeaks),
                                             1 if swap else 0, int(mode), out, _ptr(cand), _ptr(surf)), "match_ncc_full_any")
        return (out, cand, surf) if surface else (out, cand)

    def match_ncc_full_any_dev(self, d_xyuvav, n, offset, ocw, radius, npeaks, d_out, d_cand=0, d_shift=0, stream=0, swap=False, mode=0,
                               d_surf=0):
        """Device-pointer variant (enqueue only): as match_ncc_full_dn_dev; d_surf 0 = no surfaces."""
        _check(_lib.mimc3_match_ncc_full_any_dev(self._h, d_xyuvav, n, int(offset[0]), int(offset[1]), d_shift or None, ocw, radius,
                                                 npeaks, 1 if swap else 0, int(mode), d_out, d_cand or None, d_surf or None, stream),
               "match_ncc_full_any_dev")

    def match_ncc_full_chip(self, xyuvav, offset, ocw, radius, npeaks=0, shift=None, swap=False, mode=0, surface=False):
        """The exhaustive search at any chip half-width 1 <= ocw <= full_chip_max_ocw() (mimc3_match_ncc_full_chip): mode 0 at one of the
        six built chip sizes IS match_ncc_full_any(mode=0); any other ocw, and all of mode 1, runs the run-time-ocw float kernel
        ("f32g_chip") under match_ncc_full_any's mode-1 definition -> (record, candidates or None[, surfaces]) as there."""
        xy, n, out, cand, surf, fb, sh = _search_arrays("match_ncc_full_chip", xyuvav, shift, npeaks=npeaks, radius=radius, surface=surface)
        _check(_lib.mimc3_match_ncc_full_chip(self._h, xy, n, np.ascontiguousarray(offset, np.int32), _ptr(sh), ocw, radius, int(npeaks),
                                              1 if swap else 0, int(mode), out, _ptr(cand), _ptr(surf)), "match_ncc_full_chip")
        return (out, cand, surf) if surface else (out, cand)

    def match_ncc_full_chip_dev(self, d_xyuvav, n, offset, ocw, radius, npeaks, d_out, d_cand=0, d_shift=0, stream=0, swap=False, mode=0,
                                d_surf=0):
        """Device-pointer variant (enqueue only): as match_ncc_full_any_dev."""
        _check(_lib.mimc3_match_ncc_full_chip_dev(self._h, d_xyuvav, n, int(offset[0]), int(offset[1]), d_shift or None, ocw, radius,
                                                  npeaks, 1 if swap else 0, int(mode), d_out, d_cand or None, d_surf or None, stream),
               "match_ncc_full_chip_dev")

    def match_ncc_full_chip_class(self, xyuvav, offset, ocw, radius, npeaks=0, shift=None, swap=False, mode=0, surface=False):
        """match_ncc_full_chip with the 8-bit pair on the matrix cores at every chip size (mimc3_match_ncc_full_chip_class): mode 0 at one of
        the six built chip sizes is the class dispatch ("u8_mfma_full", "u16_full", "f32i_full", "f32g_full"; the surfaces as
        match_ncc_full_surf serves them); at any other ocw an 8-bit pair runs the run-time-ocw matrix-core kernel ("u8_mfma_chip") and
        every other class the float kernel ("f32g_chip"); mode 1 runs the matrix-core kernel at every ocw and takes 8-bit pairs only.
        On an 8-bit pair the bytes are match_ncc_full_chip(mode=1)'s -> (record, candidates or None[, surfaces]) as there."""
        xy, n, out, cand, surf, fb, sh = _search_arrays("match_ncc_full_chip_class", xyuvav, shift, npeaks=npeaks, radius=radius, surface=surface)
        _check(_lib.mimc3_match_ncc_full_chip_class(self._h, xy, n, np.ascontiguousarray(offset, np.int32), _ptr(sh), ocw, radius, int(npeaks),
                                                    1 if swap else 0, int(mode), out, _ptr(cand), _ptr(surf)), "match_ncc_full_chip_class")
        return (out, cand, surf) if surface else (out, cand)

    def match_ncc_full_chip_class_dev(self, d_xyuvav, n, offset, ocw, radius, npeaks, d_out, d_cand=0, d_shift=0, stream=0, swap=False, mode=0,
                                      d_surf=0):
        """Device-pointer variant (enqueue only): as match_ncc_full_chip_dev."""
        _check(_lib.mimc3_match_ncc_full_chip_class_dev(self._h, d_xyuvav, n, int(offset[0]), int(offset[1]), d_shift or None, ocw, radius,
                                                        npeaks, 1 if swap else 0, int(mode), d_out, d_cand or None, d_surf or None, stream),
               "match_ncc_full_chip_class_dev")

    def match_ncc_full_chip_planes(self, xyuvav, offset, ocw, radius, npeaks=0, shift=None, swap=False, mode=0, surface=False):
        """match_ncc_full_chip with the 8-bit and the scaled-integer pair (12-bit DN, a filtered 8-bit pair) on the matrix cores at every chip
        size (mimc3_match_ncc_full_chip_planes): mode 0 at one of the six built chip sizes is the class dispatch, as
        match_ncc_full_chip_class(mode=0); at any other ocw an 8-bit pair runs "u8_mfma_chip", a scaled-integer pair the run-time-ocw
        matrix-core kernel on the u16 planes ("u16_mfma_chip") and every other class the float kernel ("f32g_chip"); mode 1 runs
        "u16_mfma_chip" at every ocw and takes 8-bit and scaled-integer pairs only.  On such a pair the bytes are
        match_ncc_full_chip(mode=1)'s -> (record, candidates or None[, surfaces]) as there."""
        xy, n, out, cand, surf, fb, sh = _search_arrays("match_ncc_full_chip_planes", xyuvav, shift, npeaks=npeaks, radius=radius, surface=surface)
        _check(_lib.mimc3_match_ncc_full_chip_planes(self._h, xy, n, np.ascontiguousarray(offset, np.int32), _ptr(sh), ocw, radius, int(npeaks),
                                                     1 if swap else 0, int(mode), out, _ptr(cand), _ptr(surf)), "match_ncc_full_chip_planes")
        return (out, cand, surf) if surface else (out, cand)

    def match_ncc_full_chip_planes_dev(self, d_xyuvav, n, offset, ocw, radius, npeaks, d_out, d_cand=0, d_shift=0, stream=0, swap=False, mode=0,
                                       d_surf=0):
        """Device-pointer variant (enqueue only): as match_ncc_full_chip_dev."""
        _check(_lib.mimc3_match_ncc_full_chip_planes_dev(self._h, d_xyuvav, n, int(offset[0]), int(offset[1]), d_shift or None, ocw, radius,
                                                         npeaks, 1 if swap else 0, int(mode), d_out, d_cand or None, d_surf or None, stream),
               "match_ncc_full_chip_planes_dev")

    def match_ncc_full_surf(self, xyuvav, offset, ocw, radius, npeaks=0, shift=None, swap=False):
        """The exhaustive search with every point's NCC surface from the kernel of the pair's class (mimc3_match_ncc_full_surf): the
        dispatch of match_ncc_full_any(mode=0) -- "u8_mfma_full", "u16_full", "f32i_full" or "f32g_full" -- with the surfaces served by
        whichever kernel runs -> (float32[N][8] record and float32[npeaks][N][3] candidates or None when npeaks == 0, exactly
        match_ncc_full_dn's on an integer-class pair, float32[N][(2 radius + 1)^2] surfaces in k order).  The surface equals
        match_ncc_full_any(mode=1, surface=True)'s cell for cell as f32 values (finite cells bit for bit, a non-finite cell of the same
        kind; NaN payloads are not part of the contract)."""
        xy, n, out, cand, surf, fb, sh = _search_arrays("match_ncc_full_surf", xyuvav, shift, npeaks=npeaks, radius=radius, surface=True)
        _check(_lib.mimc3_match_ncc_full_surf(self._h, xy, n, np.ascontiguousarray(offset, np.int32), _ptr(sh), ocw, radius, int(npeaks),
                                              1 if swap else 0, out, _ptr(cand), _ptr(surf)), "match_ncc_full_surf")
        return out, cand, surf

    def match_ncc_full_surf_dev(self, d_xyuvav, n, offset, ocw, radius, npeaks, d_out, d_surf, d_cand=0, d_shift=0, stream=0, swap=False):
        """Device-pointer variant (enqueue only): as match_ncc_full_any_dev without mode; d_surf float32[n][(2 radius + 1)^2] is required."""
        _check(_lib.mimc3_match_ncc_full_surf_dev(self._h, d_xyuvav, n, int(offset[0]), int(offset[1]), d_shift or None, ocw, radius,
                                                  npeaks, 1 if swap else 0, d_out, d_cand or None, d_surf or None, stream),
               "match_ncc_full_surf_dev")

    def match_ncc_wide(self, xyuvav, offset, ocw, radius, npeaks=0, shift=None, swap=False, surface=False):
        """The exhaustive search beyond +-15 px (mimc3_match_ncc_wide): match_ncc_full_any(mode=1) with 1 <= radius <=
        wide_max_radius(ocw) -- up to +-47 px in one exact pass at full resolution, candidates from the whole range.  radius <= 15 is
        that call, byte for byte ("f32g_full"); radius >= 16 runs the wide kernel ("f32g_wide") -> (float32[N][8] record,
        float32[npeaks][N][3] candidates or None when npeaks == 0), and with surface=True every point's NCC surface
        float32[N][(2 radius + 1)^2] in k order as a third item."""
        xy, n, out, cand, surf, fb, sh = _search_arrays("match_ncc_wide", xyuvav, shift, npeaks=npeaks, radius=radius, surface=surface)
        _check(_lib.mimc3_match_ncc_wide(self._h, xy, n, np.ascontiguousarray(offset, np.int32),
                                         _ptr(sh), ocw, radius, int(npeaks), 1 if swap else 0, out, _ptr(cand), _ptr(surf)), "match_ncc_wide")
        return (out, cand, surf) if surface else (out, cand)

    def match_ncc_wide_dev(self, d_xyuvav, n, offset, ocw, radius, npeaks, d_out, d_cand=0, d_shift=0, stream=0, swap=False, d_surf=0):
        """Device-pointer variant (enqueue only): as match_ncc_full_any_dev; d_surf 0 = no surfaces."""
        _check(_lib.mimc3_match_ncc_wide_dev(self._h, d_xyuvav, n, int(offset[0]), int(offset[1]), d_shift or None, ocw, radius,
                                             npeaks, 1 if swap else 0, d_out, d_cand or None, d_surf or None, stream),
               "match_ncc_wide_dev")

    def match_ncc_wide_class(self, xyuvav, offset, ocw, radius, npeaks=0, shift=None, swap=False, mode=0, surface=False):
        """The exhaustive search beyond +-15 px with the 8-bit pair on the matrix cores at every chip half-width 1..80
        (mimc3_match_ncc_wide_class), 1 <= radius <= wide_class_max_radius(ocw).  radius <= 15 is match_ncc_full_chip_class with the same
        mode, byte for byte.  radius >= 16: mode 1 runs the matrix-core wide kernel ("u8_mfma_wide") and takes 8-bit pairs only; mode 0
        runs it on an 8-bit pair and the float wide kernel ("f32g_wide") on any other pair, where match_ncc_wide takes (ocw, radius).
        On an 8-bit pair the bytes are match_ncc_wide's -> (record, candidates or None[, surfaces]) as there."""
        xy, n, out, cand, surf, fb, sh = _search_arrays("match_ncc_wide_class", xyuvav, shift, npeaks=npeaks, radius=radius, surface=surface)
        _check(_lib.mimc3_match_ncc_wide_class(self._h, xy, n, np.ascontiguousarray(offset, np.int32), _ptr(sh), ocw, radius, int(npeaks),
                                               1 if swap else 0, int(mode), out, _ptr(cand), _ptr(surf)), "match_ncc_wide_class")
        return (out, cand, surf) if surface else (out, cand)

    def match_ncc_wide_class_dev(self, d_xyuvav, n, offset, ocw, radius, npeaks, d_out, d_cand=0, d_shift=0, stream=0, swap=False, mode=0,
                                 d_surf=0):
        """Device-pointer variant (enqueue only): as match_ncc_full_chip_dev."""
        _check(_lib.mimc3_match_ncc_wide_class_dev(self._h, d_xyuvav, n, int(offset[0]), int(offset[1]), d_shift or None, ocw, radius,
                                                   npeaks, 1 if swap else 0, int(mode), d_out, d_cand or None, d_surf or None, stream),
               "match_ncc_wide_class_dev")

    def match_ncc_wide_planes(self, xyuvav, offset, ocw, radius, npeaks=0, shift=None, swap=False, mode=0, surface=False):
        """The exhaustive search beyond +-15 px with the 8-bit AND the scaled-integer pair (12-bit DN, a filtered 8-bit pair) on the matrix
        cores at every chip half-width 1..80 (mimc3_match_ncc_wide_planes), 1 <= radius <= wide_class_max_radius(ocw).  radius <= 15 is
        match_ncc_full_chip_planes with the same mode, byte for byte.  radius >= 16: mode 1 runs the matrix-core wide kernel on the u16
        planes ("u16_mfma_wide") up to wide_planes_max_radius(ocw) and takes 8-bit and scaled-integer pairs only; mode 0 sends an 8-bit
        pair where match_ncc_wide_class does, runs a scaled-integer pair on "u16_mfma_wide" (or on "f32g_wide" beyond its radius, where
        match_ncc_wide takes (ocw, radius)) and any other pair as match_ncc_wide_class does.  The bytes are match_ncc_wide's
        -> (record, candidates or None[, surfaces]) as there."""
        xy, n, out, cand, surf, fb, sh = _search_arrays("match_ncc_wide_planes", xyuvav, shift, npeaks=npeaks, radius=radius, surface=surface)
        _check(_lib.mimc3_match_ncc_wide_planes(self._h, xy, n, np.ascontiguousarray(offset, np.int32), _ptr(sh), ocw, radius, int(npeaks),
                                                1 if swap else 0, int(mode), out, _ptr(cand), _ptr(surf)), "match_ncc_wide_planes")
        return (out, cand, surf) if surface else (out, cand)

    def match_ncc_wide_planes_dev(self, d_xyuvav, n, offset, ocw, radius, npeaks, d_out, d_cand=0, d_shift=0, stream=0, swap=False, mode=0,
                                  d_surf=0):
        """Device-pointer variant (enqueue only): as match_ncc_full_chip_dev."""
        _check(_lib.mimc3_match_ncc_wide_planes_dev(self._h, d_xyuvav, n, int(offset[0]), int(offset[1]), d_shift or None, ocw, radius,
                                                    npeaks, 1 if swap else 0, int(mode), d_out, d_cand or None, d_surf or None, stream),
               "match_ncc_wide_planes_dev")

    def match_ncc_wide_chip(self, xyuvav, offset, ocw, radius, npeaks=0, shift=None, swap=False, mode=0, surface=False):
        """The exhaustive search beyond +-15 px on ANY pair -- 16-bit DN, float pixels, NaN or negative nulls -- at every chip half-width
        1..80 (mimc3_match_ncc_wide_chip), 1 <= radius <= wide_chip_max_radius(ocw) = 47.  Mode 1 is match_ncc_full_any(mode=1)'s
        definition on the run-time-ocw kernels: radius <= 15 is match_ncc_full_chip(mode=1), byte for byte ("f32g_chip"); radius >= 16
        runs the run-time-ocw wide float kernel ("f32g_wide_chip").  Mode 0 refuses no pair and no (ocw, radius) in range: radius <= 15
        is match_ncc_full_chip_planes(mode=0); radius >= 16 goes where match_ncc_wide_class / match_ncc_wide_planes (mode 0) send an
        8-bit / scaled-integer pair, to "f32g_wide" where match_ncc_wide takes (ocw, radius), and to "f32g_wide_chip" everywhere else
        (wide_chip_path has the table) -> (record, candidates or None[, surfaces]) as match_ncc_wide."""
        xy, n, out, cand, surf, fb, sh = _search_arrays("match_ncc_wide_chip", xyuvav, shift, npeaks=npeaks, radius=radius, surface=surface)
        _check(_lib.mimc3_match_ncc_wide_chip(self._h, xy, n, np.ascontiguousarray(offset, np.int32), _ptr(sh), ocw, radius, int(npeaks),
                                              1 if swap else 0, int(mode), out, _ptr(cand), _ptr(surf)), "match_ncc_wide_chip")
        return (out, cand, surf) if surface else (out, cand)

    def match_ncc_wide_chip_dev(self, d_xyuvav, n, offset, ocw, radius, npeaks, d_out, d_cand=0, d_shift=0, stream=0, swap=False, mode=0,
                                d_surf=0):
        """Device-pointer variant (enqueue only): as match_ncc_full_chip_dev."""
        _check(_lib.mimc3_match_ncc_wide_chip_dev(self._h, d_xyuvav, n, int(offset[0]), int(offset[1]), d_shift or None, ocw, radius,
                                                  npeaks, 1 if swap else 0, int(mode), d_out, d_cand or None, d_surf or None, stream),
               "match_ncc_wide_chip_dev")

    def match_ncc_full_fb(self, xyuvav, offset, ocw, radius, npeaks=0, shift=None, mode=0):
        """Forward-backward consistency of the exhaustive search (mimc3_match_ncc_full_fb): the forward pass is match_ncc_full_any(swap
        False, mode), bit for bit; every forward result -- the record and each of the npeaks candidates -- is then matched back from
        where it landed (chip from i1, search in i0) in one backward pass on the device -> (float32[N][8] record,
        float32[npeaks][N][3] candidates or None when npeaks == 0, float32[1 + npeaks][N][4] fb).  An fb row is (du_b, dv_b, ncc_b, err),
        err = |d_forward + d_backward| (near 0 for a reciprocal peak); column 2 holds a status where there is no row: -5 the forward
        result has no fit, -6 the chip at the landing point leaves the image, -2 / -3 / -4 the backward search's own."""
        xy, n, out, cand, surf, fb, sh = _search_arrays("match_ncc_full_fb", xyuvav, shift, npeaks=npeaks, fb=True)
        _check(_lib.mimc3_match_ncc_full_fb(self._h, xy, n, np.ascontiguousarray(offset, np.int32),
                                            _ptr(sh), ocw, radius, int(npeaks), int(mode), out, _ptr(cand), _ptr(fb)), "match_ncc_full_fb")
        return out, cand, fb

    def match_ncc_full_fb_dev(self, d_xyuvav, n, offset, ocw, radius, npeaks, d_out, d_fb, d_cand=0, d_shift=0, stream=0, mode=0):
        """Device-pointer variant (enqueue only): as match_ncc_full_any_dev, plus d_fb float32[1 + npeaks][n][4]."""
        _check(_lib.mimc3_match_ncc_full_fb_dev(self._h, d_xyuvav, n, int(offset[0]), int(offset[1]), d_shift or None, ocw, radius,
                                                npeaks, int(mode), d_out, d_cand or None, d_fb, stream),
               "match_ncc_full_fb_dev")

    def match_ncc_wide_fb(self, xyuvav, offset, ocw, radius, npeaks=0, shift=None):
        """Forward-backward consistency beyond +-15 px (mimc3_match_ncc_wide_fb): match_ncc_full_fb under match_ncc_wide's definition, 1 <=
        radius <= wide_max_radius(ocw) -- the forward pass is match_ncc_wide(swap False), the one backward pass match_ncc_wide(swap True)
        over the record and the candidates of every point -> (float32[N][8] record, float32[npeaks][N][3] candidates or None when
        npeaks == 0, float32[1 + npeaks][N][4] fb); radius <= 15 returns the bytes of match_ncc_full_fb(mode=1)."""
        xy, n, out, cand, surf, fb, sh = _search_arrays("match_ncc_wide_fb", xyuvav, shift, npeaks=npeaks, fb=True)
        _check(_lib.mimc3_match_ncc_wide_fb(self._h, xy, n, np.ascontiguousarray(offset, np.int32),
                                            _ptr(sh), ocw, radius, int(npeaks), out, _ptr(cand), _ptr(fb)), "match_ncc_wide_fb")
        return out, cand, fb

    def match_ncc_wide_fb_dev(self, d_xyuvav, n, offset, ocw, radius, npeaks, d_out, d_fb, d_cand=0, d_shift=0, stream=0):
        """Device-pointer variant (enqueue only): as match_ncc_wide_dev, plus d_fb float32[1 + npeaks][n][4]."""
        _check(_lib.mimc3_match_ncc_wide_fb_dev(self._h, d_xyuvav, n, int(offset[0]), int(offset[1]), d_shift or None, ocw, radius,
                                                npeaks, d_out, d_cand or None, d_fb, stream),
               "match_ncc_wide_fb_dev")

    # ---- NCC stacking (mimc3_stack_*): the surfaces of several pairs averaged per cell, the peak searched once on the mean ----
    def stack_begin(self, n, radius, shift=None):
        """Size and zero the context's stack for n grid points and search radius `radius` (1..15); shift int32[n][2] is the search shift
        of every layer (None = zero).  A second call discards the first stack, n = 0 releases its memory.  The stack outlives the pair:
        set_images and filter_images leave it alone."""
        n = int(n)
        sh = None
        if shift is not None and n > 0:
            sh = np.ascontiguousarray(shift, np.int32)
            if sh.shape != (n, 2):
                raise ValueError(f"stack_begin: shift must be int32[{n}][2], got {sh.shape}")
        _check(_lib.mimc3_stack_begin(self._h, n, int(radius), _ptr(sh)), "stack_begin")

    def stack_begin_wide(self, n, radius, shift=None):
        """stack_begin with radius 1..47 (mimc3_stack_begin_wide).  radius <= 15 leaves the context exactly as stack_begin does; on a
        stack of radius >= 16 a layer of stack_add is match_ncc_wide's surface (an ocw with radius > wide_max_radius(ocw) is refused) and
        stack_finish runs that entry's tail."""
        n = int(n)
        sh = None
        if shift is not None and n > 0:
            sh = np.ascontiguousarray(shift, np.int32)
            if sh.shape != (n, 2):
                raise ValueError(f"stack_begin_wide: shift must be int32[{n}][2], got {sh.shape}")
        _check(_lib.mimc3_stack_begin_wide(self._h, n, int(radius), _ptr(sh)), "stack_begin_wide")

    def stack_add(self, xyuvav, offset, ocw, swap=False):
        """One layer from the resident pair: the surfaces of match_ncc_full_any(mode=1) with the stack's shift and radius, accumulated
        cell by cell (finite cells only); a point that call refuses (status -3) does not count as a layer of that point."""
        xy = np.ascontiguousarray(xyuvav, np.float64)
        _check(_lib.mimc3_stack_add(self._h, xy, xy.shape[0], np.ascontiguousarray(offset, np.int32), ocw, 1 if swap else 0), "stack_add")

    def stack_add_dev(self, d_xyuvav, n, offset, ocw, stream=0, swap=False):
        """Device-pointer variant (enqueue only)."""
        _check(_lib.mimc3_stack_add_dev(self._h, d_xyuvav, n, int(offset[0]), int(offset[1]), ocw, 1 if swap else 0, stream), "stack_add_dev")

    def stack_add_class(self, xyuvav, offset, ocw, swap=False):
        """stack_add through the kernel of the pair's class (mimc3_stack_add_class): on a stack of radius <= 15 the layer's surfaces are
        match_ncc_full_surf's -- the matrix cores on an 8-bit pair, the u16 or f32 planes' kernels on 12- and 16-bit DN -- and the
        stack's state afterwards is bit for bit stack_add's; on a stack of radius >= 16 it is stack_add."""
        xy = np.ascontiguousarray(xyuvav, np.float64)
        _check(_lib.mimc3_stack_add_class(self._h, xy, xy.shape[0], np.ascontiguousarray(offset, np.int32), ocw, 1 if swap else 0),
               "stack_add_class")

    def stack_add_class_dev(self, d_xyuvav, n, offset, ocw, stream=0, swap=False):
        """Device-pointer variant (enqueue only)."""
        _check(_lib.mimc3_stack_add_class_dev(self._h, d_xyuvav, n, int(offset[0]), int(offset[1]), ocw, 1 if swap else 0, stream),
               "stack_add_class_dev")

    def stack_add_fused(self, xyuvav, offset, ocw, swap=False):
        """One layer from the resident pair at any chip half-width 1..80 and any stack radius up to stack_fused_max_radius(ocw)
        (mimc3_stack_add_fused): the layer is match_ncc_wide_planes(mode=0, surface=True) with the stack's shift and radius, added as
        stack_add_surfaces adds it -- the stack afterwards is bit for bit that chain's, and stack_add's at the six chip sizes.  An 8-bit
        or scaled-integer pair runs the accumulating forms of the run-time-ocw matrix-core kernels ("u8_mfma_chip" / "u8_mfma_wide",
        "u16_mfma_chip" / "u16_mfma_wide"): one launch pair over all points that adds every surface into the stack from LDS, with no
        layer scratch and no chunks; any other pair goes through the layer scratch on the kernel that entry runs.  last_path() reports
        the kernel."""
        xy = np.ascontiguousarray(xyuvav, np.float64)
        _check(_lib.mimc3_stack_add_fused(self._h, xy, xy.shape[0], np.ascontiguousarray(offset, np.int32), ocw, 1 if swap else 0),
               "stack_add_fused")

    def stack_add_fused_dev(self, d_xyuvav, n, offset, ocw, stream=0, swap=False):
        """Device-pointer variant (enqueue only)."""
        _check(_lib.mimc3_stack_add_fused_dev(self._h, d_xyuvav, n, int(offset[0]), int(offset[1]), ocw, 1 if swap else 0, stream),
               "stack_add_fused_dev")

    def stack_fused_max_radius(self, ocw):
        """The largest stack radius stack_add_fused takes for the resident pair's class at this ocw: 47 on an 8-bit pair,
        wide_planes_max_radius(ocw) on a scaled-integer one, else 15, or wide_max_radius(ocw) at the six chip sizes; 0 for an ocw
        outside 1..80 or without a pair.  Also the largest LAYER radius stack_add_scaled_fused takes, whatever the stack's radius."""
        return int(_lib.mimc3_stack_fused_max_radius(self._h, int(ocw)))

    def stack_add_surfaces(self, surf, refused=None):
        """One layer from the caller's surfaces float32[n][(2 radius + 1)^2] in k order; refused bool[n] (None = no point is)."""
        sf = np.ascontiguousarray(surf, np.float32)
        if sf.ndim != 2:
            raise ValueError(f"stack_add_surfaces: surf must be float32[n][cells], got {sf.shape}")
        n, r = self.stack_info()[:2]
        if n and sf.shape[1] != (2 * r + 1) ** 2:
            raise ValueError(f"stack_add_surfaces: surf must have {(2 * r + 1) ** 2} cells per point, got {sf.shape[1]}")
        rf = None
        if refused is not None:
            rf = np.ascontiguousarray(np.asarray(refused) != 0, np.uint8)
            if rf.shape != (sf.shape[0],):
                raise ValueError(f"stack_add_surfaces: refused must be [{sf.shape[0]}], got {rf.shape}")
        _check(_lib.mimc3_stack_add_surfaces(self._h, sf, None if rf is None else rf.ctypes.data, sf.shape[0]), "stack_add_surfaces")

    def stack_add_surfaces_dev(self, d_surf, n, d_refused=0, stream=0):
        """Device-pointer variant (enqueue only): d_surf float32[n][cells], d_refused uint8[n] or 0."""
        _check(_lib.mimc3_stack_add_surfaces_dev(self._h, d_surf, d_refused or None, n, stream), "stack_add_surfaces_dev")

    # ---- layers of another time baseline: a pair `scale` times as long as the stack's moved scale x as far ----
    def stack_layer_shift(self, scale):
        """int32[n][2]: the shift a layer at `scale` is searched around, rint(scale * the stack's shift) (mimc3_stack_layer_shift)."""
        out = np.empty((self.stack_info()[0], 2), np.int32)
        _check(_lib.mimc3_stack_layer_shift(self._h, float(scale), out), "stack_layer_shift")
        return out

    def stack_weighted(self):
        """True once a layer with a weight other than 1 was added: the stack then keeps the weights' sum per cell (18 bytes per cell)."""
        return bool(_lib.mimc3_stack_weighted(self._h))

    def _scaled_radius(self, what, scale, radius, ocw):
        if radius is not None:
            return int(radius)
        r = stack_layer_radius(self.stack_info()[1], scale)
        if r > wide_max_radius(ocw):
            raise ValueError(f"{what}: scale {scale} wants a layer radius of {r}, beyond wide_max_radius({ocw}) = {wide_max_radius(ocw)}: "
                             f"pass a radius explicitly (the stack's outer cells then get no count from this layer)")
        return r

    def stack_add_scaled(self, xyuvav, offset, ocw, scale, weight=1.0, radius=None, swap=False):
        """One layer from the resident pair, whose time separation is `scale` times the stack's: match_ncc_wide's surfaces at `radius`
        (None: stack_layer_radius of the stack's radius) around stack_layer_shift(scale), resampled bilinearly onto the stack's cells
        and accumulated with `weight` (mimc3_stack_add_scaled)."""
        xy = np.ascontiguousarray(xyuvav, np.float64)
        r = self._scaled_radius("stack_add_scaled", scale, radius, ocw)
        _check(_lib.mimc3_stack_add_scaled(self._h, xy, xy.shape[0], np.ascontiguousarray(offset, np.int32), ocw, r, 1 if swap else 0,
                                           float(scale), float(weight)), "stack_add_scaled")

    def stack_add_scaled_dev(self, d_xyuvav, n, offset, ocw, scale, weight=1.0, radius=None, stream=0, swap=False):
        """Device-pointer variant (enqueue only)."""
        r = self._scaled_radius("stack_add_scaled_dev", scale, radius, ocw)
        _check(_lib.mimc3_stack_add_scaled_dev(self._h, d_xyuvav, n, int(offset[0]), int(offset[1]), ocw, r, 1 if swap else 0, float(scale),
                                               float(weight), stream), "stack_add_scaled_dev")

    def _scaled_fused_radius(self, what, scale, radius, ocw):
        if radius is not None:
            return int(radius)
        r, lim = stack_layer_radius(self.stack_info()[1], scale), self.stack_fused_max_radius(ocw)
        if r > lim:
            raise ValueError(f"{what}: scale {scale} wants a layer radius of {r}, beyond stack_fused_max_radius({ocw}) = {lim}: "
                             f"pass a radius explicitly (the stack's outer cells then get no count from this layer)")
        return r

    def stack_add_scaled_fused(self, xyuvav, offset, ocw, scale, weight=1.0, radius=None, swap=False):
        """stack_add_scaled at any chip half-width 1..80 and any layer radius up to stack_fused_max_radius(ocw), resampled in the
        search's own tail (mimc3_stack_add_scaled_fused): the layer is match_ncc_wide_planes(mode=0, surface=True) at `radius` (None:
        stack_layer_radius of the stack's radius) around stack_layer_shift(scale), added as stack_add_surfaces_scaled adds it -- the
        stack afterwards is bit for bit that chain's, and stack_add_scaled's at the six chip sizes.  An 8-bit or scaled-integer pair
        runs the accumulating forms of the run-time-ocw matrix-core kernels ("u8_mfma_chip" / "u8_mfma_wide", "u16_mfma_chip" /
        "u16_mfma_wide"): one launch pair over all points, every workgroup resampling its point's surface from LDS into the stack,
        with no layer scratch and no chunks; any other pair goes through the layer scratch on the kernel that entry runs.
        last_path() reports the kernel."""
        xy = np.ascontiguousarray(xyuvav, np.float64)
        r = self._scaled_fused_radius("stack_add_scaled_fused", scale, radius, ocw)
        _check(_lib.mimc3_stack_add_scaled_fused(self._h, xy, xy.shape[0], np.ascontiguousarray(offset, np.int32), ocw, r, 1 if swap else 0,
                                                 float(scale), float(weight)), "stack_add_scaled_fused")

    def stack_add_scaled_fused_dev(self, d_xyuvav, n, offset, ocw, scale, weight=1.0, radius=None, stream=0, swap=False):
        """Device-pointer variant (enqueue only)."""
        r = self._scaled_fused_radius("stack_add_scaled_fused_dev", scale, radius, ocw)
        _check(_lib.mimc3_stack_add_scaled_fused_dev(self._h, d_xyuvav, n, int(offset[0]), int(offset[1]), ocw, r, 1 if swap else 0,
                                                     float(scale), float(weight), stream), "stack_add_scaled_fused_dev")

    def stack_add_surfaces_scaled(self, surf, radius, scale, weight=1.0, refused=None):
        """One scaled layer from the caller's surfaces float32[n][(2 radius + 1)^2] in k order, searched around
        stack_layer_shift(scale); refused bool[n] (None = no point is)."""
        sf = np.ascontiguousarray(surf, np.float32)
        radius = int(radius)
        if sf.ndim != 2 or (1 <= radius <= 47 and sf.shape[1] != (2 * radius + 1) ** 2):
            raise ValueError(f"stack_add_surfaces_scaled: surf must be float32[n][(2 radius + 1)^2], got {sf.shape} at radius {radius}")
        rf = None
        if refused is not None:
            rf = np.ascontiguousarray(np.asarray(refused) != 0, np.uint8)
            if rf.shape != (sf.shape[0],):
                raise ValueError(f"stack_add_surfaces_scaled: refused must be [{sf.shape[0]}], got {rf.shape}")
        _check(_lib.mimc3_stack_add_surfaces_scaled(self._h, sf, None if rf is None else rf.ctypes.data, sf.shape[0], radius, float(scale),
                                                    float(weight)), "stack_add_surfaces_scaled")

    def stack_add_surfaces_scaled_dev(self, d_surf, n, radius, scale, weight=1.0, d_refused=0, stream=0):
        """Device-pointer variant (enqueue only): d_surf float32[n][(2 radius + 1)^2], d_refused uint8[n] or 0."""
        _check(_lib.mimc3_stack_add_surfaces_scaled_dev(self._h, d_surf, d_refused or None, n, int(radius), float(scale), float(weight),
                                                        stream), "stack_add_surfaces_scaled_dev")

    def stack_finish(self, npeaks=0, min_count=1, surface=False):
        """The result of the stack -> (float32[n][8] record, float32[npeaks][n][3] candidates or None when npeaks == 0, uint16[n] layers
        per point[, float32[n][cells] mean surface with surface=True]): the tail of the exhaustive search over the mean surface, a
        cell being the mean of its finite values where at least min_count layers had one and NaN elsewhere; status -3 for a point no
        layer took.  Leaves the stack unchanged: more layers may follow."""
        n, r, _ = self.stack_info()
        npeaks = int(npeaks)
        out = np.empty((n, 8), np.float32)
        cand = np.empty((npeaks, n, 3), np.float32) if npeaks > 0 else None
        count = np.empty(n, np.uint16)
        surf = np.empty((n, (2 * r + 1) ** 2), np.float32) if surface else None
        _check(_lib.mimc3_stack_finish(self._h, npeaks, int(min_count), out, _ptr(cand),
                                       _ptr(surf), count.ctypes.data), "stack_finish")
        return (out, cand, count, surf) if surface else (out, cand, count)

    def stack_finish_dev(self, npeaks, min_count, d_out, d_cand=0, d_surf=0, d_count=0, stream=0):
        """Device-pointer variant (enqueue only): d_out float32[n][8], d_cand float32[npeaks][n][3] (0 iff npeaks == 0), d_surf
        float32[n][cells] or 0, d_count uint16[n] or 0."""
        _check(_lib.mimc3_stack_finish_dev(self._h, int(npeaks), int(min_count), d_out, d_cand or None, d_surf or None, d_count or None,
                                           stream), "stack_finish_dev")

    def stack_info(self):
        """(n, radius, layers) of the context's stack; (0, 0, 0) without one."""
        n, r, k = C.c_int32(), C.c_int32(), C.c_int32()
        _check(_lib.mimc3_stack_info(self._h, C.byref(n), C.byref(r), C.byref(k)), "stack_info")
        return n.value, r.value, k.value

    def full_candidates(self, xyuvav, offset, vec_ocw, radius, npeaks, kernels=(None,) + CLI_KERNELS, shift=None, any_pair=False,
                        any_ocw=False, levels=1):
        """The candidates of the exhaustive search over image variants and chip sizes -> dp float32[ndp][N][3], ndp = len(kernels) *
        len(vec_ocw) * npeaks <= 64: for each variant in order (None = the raw pair, else filter_images(kernel)) and each ocw one
        forward match_ncc_full_dn call, its candidates stacked variant-major, then ocw, then peak rank -- what
        calc_mean_var_num_dp_cluster and mimc2_postprocess read.  Every variant is filtered from fresh planes (see filter_images).
        The pair is left unfiltered.  any_pair: the calls are match_ncc_full_any's (mode 0), so a float pair goes through every variant.
        any_ocw: the calls are match_ncc_full_chip's (mode 0), so vec_ocw may hold any chip half-width 1 .. full_chip_max_ocw() -- the
        reference's (7, 10, 15, 11) and (14, 30, 60, 80) -- and any pair; at a chip size in range other than the six built ones they are
        match_ncc_full_chip_planes's (mode 0: an 8-bit or scaled-integer pair on the matrix cores, the same bytes).  any_ocw with
        radius > 15 (up to wide_chip_max_radius(ocw), levels = 1): every call is match_ncc_wide_chip's (mode 0), any pair at any ocw.
        levels > 1: every (variant, ocw) call is match_ncc_pyramid_chip's (mode 0) over that many levels, whatever any_pair and any_ocw
        say -- any chip half-width 1 .. full_chip_max_ocw(), any pair; filter, then reduce: the levels are rebuilt after each
        filter_images.  levels = 1 runs exactly the single-level calls above."""
        levels = int(levels)
        if levels < 1:
            raise ValueError("full_candidates: levels must be at least 1")
        match = self.match_ncc_full_chip if any_ocw else self.match_ncc_full_any if any_pair else self.match_ncc_full_dn
        six = (7, 15, 16, 30, 32, 40)
        kernels = tuple(kernels); vec_ocw = tuple(int(o) for o in vec_ocw); npeaks = int(npeaks)
        ndp = len(kernels) * len(vec_ocw) * npeaks
        if npeaks < 1 or ndp < 1:
            raise ValueError("full_candidates: npeaks, kernels and vec_ocw must not be empty")
        if ndp > 64:
            raise ValueError(f"full_candidates: ndp = {len(kernels)} x {len(vec_ocw)} x {npeaks} = {ndp} > 64")
        blocks = []
        try:
            for k in kernels:
                self.filter_images(None)                  # (fresh planes: see filter_images)
                if k is not None:
                    self.filter_images(k)
                for ocw in vec_ocw:
                    if levels > 1:
                        blocks.append(self.match_ncc_pyramid_chip(xyuvav, offset, ocw, radius, levels, npeaks, shift=shift)[1])
                        continue
                    call = self.match_ncc_full_chip_planes if any_ocw and ocw not in six and 1 <= ocw <= full_chip_max_ocw() else match
                    if any_ocw and int(radius) > 15:
                        call = self.match_ncc_wide_chip
                    blocks.append(call(xyuvav, offset, ocw, radius, npeaks, shift=shift)[1])
        finally:
            self.filter_images(None)
        return np.concatenate(blocks, axis=0)

    def match_ncc_pyramid(self, xyuvav, offset, ocw, radius, levels, shift=None, swap=False):
        """Coarse-to-fine exhaustive search over an image pyramid (mimc3_match_ncc_pyramid) on the resident 8-bit pair ->
        (float32[N][8] record as match_ncc_full, int32[N][2] shift_out).  The search at +-radius runs on the pair reduced levels - 1
        times first, then each finer level around twice the coarser result; the record is match_ncc_full's with shift = shift_out."""
        xy, n, out, cand, surf, fb, sh = _search_arrays("match_ncc_pyramid", xyuvav, shift)
        sh_out = np.empty((n, 2), np.int32)
        _check(_lib.mimc3_match_ncc_pyramid(self._h, xy, n, np.ascontiguousarray(offset, np.int32), _ptr(sh),
                                            ocw, radius, levels, 1 if swap else 0, out, sh_out), "match_ncc_pyramid")
        return out, sh_out

    def match_ncc_pyramid_dev(self, d_xyuvav, n, offset, ocw, radius, levels, d_out, d_shift=0, d_shift_out=0, stream=0, swap=False):
        """Device-pointer variant (enqueue only): d_xyuvav [n][6] f64, d_shift [n][2] int32 or 0, d_out [n][8] f32,
        d_shift_out [n][2] int32 or 0."""
        _check(_lib.mimc3_match_ncc_pyramid_dev(self._h, d_xyuvav, n, int(offset[0]), int(offset[1]), d_shift or None, ocw, radius, levels,
                                                1 if swap else 0, d_out, d_shift_out or None, stream), "match_ncc_pyramid_dev")

    def match_ncc_pyramid_dn(self, xyuvav, offset, ocw, radius, levels, npeaks=0, shift=None, swap=False):
        """Coarse-to-fine exhaustive search (mimc3_match_ncc_pyramid_dn) on every pair match_ncc_full_dn takes: 8-bit, scaled-integer and
        integral-f32 (16-bit DN and its filtered forms) -> (float32[N][8] record, float32[npeaks][N][3] candidates or None when
        npeaks == 0, int32[N][2] shift_out).  The levels are reductions of the pair currently matched on (filter, then reduce); record
        and candidates are match_ncc_full_dn's with shift = shift_out."""
        xy, n, out, cand, surf, fb, sh = _search_arrays("match_ncc_pyramid_dn", xyuvav, shift, npeaks=npeaks)
        sh_out = np.empty((n, 2), np.int32)
        _check(_lib.mimc3_match_ncc_pyramid_dn(self._h, xy, n, np.ascontiguousarray(offset, np.int32), _ptr(sh),
                                               ocw, radius, levels, int(npeaks), 1 if swap else 0, out,
                                               _ptr(cand), sh_out), "match_ncc_pyramid_dn")
        return out, cand, sh_out

    def match_ncc_pyramid_dn_dev(self, d_xyuvav, n, offset, ocw, radius, levels, npeaks, d_out, d_cand=0, d_shift=0, d_shift_out=0, stream=0,
                                 swap=False):
        """Device-pointer variant (enqueue only): as match_ncc_pyramid_dev, plus d_cand [npeaks][n][3] f32 (0 with npeaks == 0)."""
        _check(_lib.mimc3_match_ncc_pyramid_dn_dev(self._h, d_xyuvav, n, int(offset[0]), int(offset[1]), d_shift or None, ocw, radius, levels,
                                                   npeaks, 1 if swap else 0, d_out, d_cand or None, d_shift_out or None, stream),
               "match_ncc_pyramid_dn_dev")

    def get_pyramid_level(self, level):
        """Level `level` (1..4) of the pair currently matched on, as pixel values -> (float32[H >> level][W >> level],) * 2."""
        H, W = self.H, self.W
        l0 = np.empty((H >> level, W >> level), np.float32); l1 = np.empty_like(l0)
        _check(_lib.mimc3_ctx_get_pyramid_level(self._h, level, l0, l1), "get_pyramid_level")
        return l0, l1

    def match_ncc_pyramid_any(self, xyuvav, offset, ocw, radius, levels, npeaks=0, shift=None, swap=False, mode=0):
        """Coarse-to-fine exhaustive search (mimc3_match_ncc_pyramid_any) on any f32 pair -> (float32[N][8] record, float32[npeaks][N][3]
        candidates or None when npeaks == 0, int32[N][2] shift_out).  mode 0: match_ncc_pyramid_dn on the pairs that takes, bit for bit,
        and float levels with the float kernel ("f32g_full") on every other pair -- non-integral pixels, NaN or negative nulls; mode 1:
        the float levels and the float kernel on any pair.  Record and candidates are match_ncc_full_any's with shift = shift_out."""
        xy, n, out, cand, surf, fb, sh = _search_arrays("match_ncc_pyramid_any", xyuvav, shift, npeaks=npeaks)
        sh_out = np.empty((n, 2), np.int32)
        _check(_lib.mimc3_match_ncc_pyramid_any(self._h, xy, n, np.ascontiguousarray(offset, np.int32), _ptr(sh),
                                                ocw, radius, levels, int(npeaks), 1 if swap else 0, int(mode), out,
                                                _ptr(cand), sh_out), "match_ncc_pyramid_any")
        return out, cand, sh_out

    def match_ncc_pyramid_any_dev(self, d_xyuvav, n, offset, ocw, radius, levels, npeaks, d_out, d_cand=0, d_shift=0, d_shift_out=0, stream=0,
                                  swap=False, mode=0):
        """Device-pointer variant (enqueue only): as match_ncc_pyramid_dn_dev, plus mode."""
        _check(_lib.mimc3_match_ncc_pyramid_any_dev(self._h, d_xyuvav, n, int(offset[0]), int(offset[1]), d_shift or None, ocw, radius, levels,
                                                    npeaks, 1 if swap else 0, int(mode), d_out, d_cand or None, d_shift_out or None, stream),
               "match_ncc_pyramid_any_dev")

    def match_ncc_pyramid_chip(self, xyuvav, offset, ocw, radius, levels, npeaks=0, shift=None, swap=False, mode=0):
        """Coarse-to-fine exhaustive search at any chip half-width 1 .. full_chip_max_ocw() (mimc3_match_ncc_pyramid_chip) on any pair ->
        (float32[N][8] record, float32[npeaks][N][3] candidates or None when npeaks == 0, int32[N][2] shift_out).  The levels are those
        of the pair's class (match_ncc_pyramid_dn's, or match_ncc_pyramid_any's float levels); one run-time-ocw kernel searches all of
        them -- the matrix cores on an 8-bit or scaled-integer pair -- see pyramid_chip_path.  mode 0 keeps the templated kernels at the
        six built chip sizes except on a scaled-integer pair; mode 1 runs the run-time-ocw kernel at every ocw."""
        xy, n, out, cand, surf, fb, sh = _search_arrays("match_ncc_pyramid_chip", xyuvav, shift, npeaks=npeaks)
        sh_out = np.empty((n, 2), np.int32)
        _check(_lib.mimc3_match_ncc_pyramid_chip(self._h, xy, n, np.ascontiguousarray(offset, np.int32), _ptr(sh),
                                                 ocw, radius, levels, int(npeaks), 1 if swap else 0, int(mode), out,
                                                 _ptr(cand), sh_out), "match_ncc_pyramid_chip")
        return out, cand, sh_out

    def match_ncc_pyramid_chip_dev(self, d_xyuvav, n, offset, ocw, radius, levels, npeaks, d_out, d_cand=0, d_shift=0, d_shift_out=0, stream=0,
                                   swap=False, mode=0):
        """Device-pointer variant (enqueue only): as match_ncc_pyramid_any_dev."""
        _check(_lib.mimc3_match_ncc_pyramid_chip_dev(self._h, d_xyuvav, n, int(offset[0]), int(offset[1]), d_shift or None, ocw, radius, levels,
                                                     npeaks, 1 if swap else 0, int(mode), d_out, d_cand or None, d_shift_out or None, stream),
               "match_ncc_pyramid_chip_dev")

    def get_pyramid_level_any(self, level):
        """FLOAT level `level` (1..4) of the pair currently matched on, whatever its class (match_ncc_pyramid_any's levels: the mean of
        each 2 x 2 block's pixels >= 1e-10) -> (float32[H >> level][W >> level],) * 2."""
        H, W = self.H, self.W
        l0 = np.empty((H >> level, W >> level), np.float32); l1 = np.empty_like(l0)
        _check(_lib.mimc3_ctx_get_pyramid_level_any(self._h, level, l0, l1), "get_pyramid_level_any")
        return l0, l1

    # -- QM -----------------------------------------------------------------------------------
    def get_dpf_pseudosmoothing(self, dpf, dpf_dx, dpf_dy, ruv, mvn, nclus, xyuvav, max_sweeps=101):
        """get_dpf_pseudosmoothing (MIMC_module.c:1986-2312). Returns (dpf, dx, dy, sweeps); inputs untouched."""
        dimy, dimx = dpf.shape
        d = np.array(dpf, np.int32, order="C")
        x = np.array(dpf_dx, np.float32, order="C")
        y = np.array(dpf_dy, np.float32, order="C")
        ruv = np.ascontiguousarray(ruv, np.int32)
        mvn = np.ascontiguousarray(mvn, np.float32)
        sw = C.c_int32(0)
        _check(_lib.mimc3_qm_pseudosmooth(self._h, dimy, dimx, d.reshape(-1), x.reshape(-1), y.reshape(-1), ruv,
                                          ruv.shape[0], mvn, mvn.shape[1], np.ascontiguousarray(nclus, np.int32),
                                          np.ascontiguousarray(xyuvav, np.float64), max_sweeps, C.byref(sw)),
               "get_dpf_pseudosmoothing")
        return d, x, y, sw.value

    def qm_workspace_bytes(self, ngrid, max_sweeps):
        return int(_lib.mimc3_qm_workspace_bytes(ngrid, max_sweeps))

    def get_dpf_pseudosmoothing_dev(self, dimy, dimx, d_dpf, d_dx, d_dy, d_ruv, nn, d_mvn, kmax, d_nclus, d_xyuvav,
                                    max_sweeps, d_work, d_sweeps=None, stream=0):
        _check(_lib.mimc3_qm_pseudosmooth_dev(self._h, dimy, dimx, d_dpf, d_dx, d_dy, d_ruv, nn, d_mvn, kmax, d_nclus,
                                              d_xyuvav, max_sweeps, d_work, d_sweeps, stream), "get_dpf_pseudosmoothing_dev")

    # -- N3: the program's data path on arrays -----------------------------------------------------
    def mimc2_postprocess(self, dp, xyuvav, dimx, dimy, dt, mpp, meter_per_spacing, radius_dpf1=3.0, radius_ps=5.0,
                          qm_max_sweeps=101):
        """mimc2_postprocess (MIMC_module.c:892-990): dp [ndp][N][3] -> vxyexyqual [5][dimy][dimx] (px units)."""
        dp = np.ascontiguousarray(dp, np.float32)
        out = np.empty((5, dimy, dimx), np.float32)
        _check(_lib.mimc3_postprocess(self._h, dp, dp.shape[0], np.ascontiguousarray(xyuvav, np.float64), dimx, dimy, dt, mpp,
                                      meter_per_spacing, radius_dpf1, radius_ps, qm_max_sweeps, out.reshape(-1)), "mimc2_postprocess")
        return out

    @staticmethod
    def _vmap_params(kernels=CLI_KERNELS, cp_seed=-1, vec_ocw=(7, 15, 30, 40), aw_cre=10.0, aw_sf=1.8, radius_neighbor_dpf1=3.0,
                     radius_neighbor_ps=5.0, num_cp_max=500, num_cp_min=50, ratio_cp=0.03, thres_spd_cp=10.0, qm_max_sweeps=101):
        ks = [np.ascontiguousarray(k, np.float32) for k in kernels]
        p = VmapParams()
        p.vec_ocw[:] = list(vec_ocw)
        p.aw_cre = aw_cre; p.aw_sf = aw_sf; p.radius_neighbor_dpf1 = radius_neighbor_dpf1; p.radius_neighbor_ps = radius_neighbor_ps
        p.num_cp_max = num_cp_max; p.num_cp_min = num_cp_min; p.ratio_cp = ratio_cp; p.thres_spd_cp = thres_spd_cp
        p.cp_seed = cp_seed; p.qm_max_sweeps = qm_max_sweeps
        for i, k in enumerate(ks):
            p.kernel[i] = k.ctypes.data
            p.kdim[i][0], p.kdim[i][1] = k.shape
        return p, ks                      # ks keeps the kernel arrays alive

    @staticmethod
    def _vmap_out(r, flag, planes):
        out = dict(dimx=r.dimx, dimy=r.dimy, mpp=r.mpp, spacing_grid=r.spacing_grid, meter_per_spacing=r.meter_per_spacing,
                   cp_status=r.cp_status, offset_cp=(r.offset_cp[0], r.offset_cp[1]), cp_subint=(r.cp_subint[0], r.cp_subint[1]),
                   flag_cp=flag)
        for name, a in zip(("vx", "vy", "ex", "ey", "qual"), planes):
            out[name] = a.reshape(r.dimy, r.dimx) if r.cp_status > 0 else None
        return out

    def vmap(self, xyuvav, dt, **kw):
        """MIMC_main.c:203-402 on the resident pair (keywords: see _vmap_params; defaults = MIMC_main.c:134-194).
        Returns dict(vx, vy, ex, ey, qual [dimy][dimx], flag_cp, + the scalar fields of mimc3_vmap_result); the planes
        are None when cp_status == -1."""
        xy = np.ascontiguousarray(xyuvav, np.float64)
        n = xy.shape[0]
        p, _keep = self._vmap_params(**kw)
        planes = [np.empty(n, np.float32) for _ in range(5)]
        flag = np.zeros(n, np.uint8)
        r = VmapResult()
        _check(_lib.mimc3_vmap(self._h, xy, n, dt, C.byref(p), *planes, flag, C.byref(r)), "vmap")
        return self._vmap_out(r, flag, planes)

    def vmap_passes(self, xyuvav, dt, lo, hi, d_dp, **kw):
        """mimc3_vmap_passes: CP offset on the whole grid + the 32 passes for grid points [lo, hi) into the device tensor
        d_dp [32][hi-lo][3] (pass its data_ptr()).  Returns (VmapResult, flag_cp)."""
        xy = np.ascontiguousarray(xyuvav, np.float64)
        p, _keep = self._vmap_params(**kw)
        flag = np.zeros(xy.shape[0], np.uint8)
        r = VmapResult()
        _check(_lib.mimc3_vmap_passes(self._h, xy, xy.shape[0], dt, C.byref(p), lo, hi, d_dp, flag, C.byref(r)), "vmap_passes")
        return r, flag

    def vmap_geometry(self, xyuvav):
        xy = np.ascontiguousarray(xyuvav, np.float64)
        r = VmapResult()
        _check(_lib.mimc3_vmap_geometry(xy, xy.shape[0], C.byref(r)), "vmap_geometry")
        return r

    def vmap_cp(self, xyuvav, dt, **kw):
        """geometry + CP offset on the whole grid -> (VmapResult, flag_cp)"""
        xy = np.ascontiguousarray(xyuvav, np.float64)
        p, _keep = self._vmap_params(**kw)
        flag = np.zeros(xy.shape[0], np.uint8)
        r = VmapResult()
        _check(_lib.mimc3_vmap_cp(self._h, xy, xy.shape[0], dt, C.byref(p), flag, C.byref(r)), "vmap_cp")
        return r, flag

    def vmap_passes_points(self, xs, dt, r, d_dp, pass_stride=0, **kw):
        """the 32 passes for the grid points xs [n][6] (any subset) into the device tensor d_dp [32][pass_stride][3]"""
        xs = np.ascontiguousarray(xs, np.float64)
        p, _keep = self._vmap_params(**kw)
        _check(_lib.mimc3_vmap_passes_points(self._h, xs, xs.shape[0], dt, C.byref(p), C.byref(r), d_dp, pass_stride), "vmap_passes_points")

    def vmap_finish(self, xyuvav, dt, d_dp_full, r, flag, **kw):
        """mimc3_vmap_finish on the complete candidate tensor [32][N][3] (device pointer); same dict as vmap()."""
        xy = np.ascontiguousarray(xyuvav, np.float64)
        n = xy.shape[0]
        p, _keep = self._vmap_params(**kw)
        planes = [np.empty(n, np.float32) for _ in range(5)]
        if r.cp_status > 0:
            _check(_lib.mimc3_vmap_finish(self._h, xy, n, dt, C.byref(p), d_dp_full, *planes, C.byref(r)), "vmap_finish")
        return self._vmap_out(r, flag, planes)

    # -- N4: control-point offset -----------------------------------------------------------------
    def get_offset_image(self, xyuvav, kernels, seed=-1, vec_ocw=(7, 15, 30, 40), aw_cre=10.0, num_cp_max=500, num_cp_min=50,
                         ratio_cp=0.03, thres_spd_cp=10.0, peers=()):
        """get_offset_image (MIMC_module.c:33-492) on the resident pair. Defaults = MIMC_main.c:134-170.
        Returns (status, offset[2], flag_cp[N], info[4], sduv[2]); status 1 = ok, -1 = not enough control points.
        peers: further Contexts holding the SAME pair (other GPUs) that share the device work (mimc3_get_offset_image_multi);
        the result does not depend on them."""
        xy = np.ascontiguousarray(xyuvav, np.float64)
        ks = [np.ascontiguousarray(k, np.float32) for k in kernels]
        p = CpParams()
        p.vec_ocw[:] = list(vec_ocw)
        p.aw_cre = aw_cre; p.num_cp_max = num_cp_max; p.num_cp_min = num_cp_min
        p.ratio_cp = ratio_cp; p.thres_spd_cp = thres_spd_cp; p.seed = seed
        for i, k in enumerate(ks):
            p.kernel[i] = k.ctypes.data
            p.kdim[i][0], p.kdim[i][1] = k.shape
        off = np.zeros(2, np.int32)
        flag = np.zeros(xy.shape[0], np.uint8)
        info = np.zeros(4, np.int32)
        sduv = np.zeros(2, np.float32)
        st = C.c_int32(0)
        if peers:
            hs = (_vp * (1 + len(peers)))(self._h, *[q._h for q in peers])
            _check(_lib.mimc3_get_offset_image_multi(hs, len(hs), xy, xy.shape[0], C.byref(p), off, flag, C.byref(st), info, sduv),
                   "get_offset_image")
        else:
            _check(_lib.mimc3_get_offset_image(self._h, xy, xy.shape[0], C.byref(p), off, flag, C.byref(st), info, sduv),
                   "get_offset_image")
        return st.value, off, flag, info, sduv

    # -- N2: image pre-filter ---------------------------------------------------------------------
    def GMA_float_conv2(self, img, kernel, out=None):
        """GMA_float_conv2 (MIMC_module.c:2517-2585). `out` is in/out as in the reference (its border takes part in
        the minimum); default = a zero plane, which is what a fresh GMA_float_create gives the CLI."""
        img = np.ascontiguousarray(img, np.float32)
        kernel = np.ascontiguousarray(kernel, np.float32)
        o = np.zeros_like(img) if out is None else np.array(out, np.float32, order="C")
        _check(_lib.mimc3_float_conv2(self._h, img, img.shape[0], img.shape[1], kernel, kernel.shape[0], kernel.shape[1], o),
               "GMA_float_conv2")
        return o

    def GMA_float_conv2_dev(self, d_in, H, W, kernel, d_out, d_scratch, stream=0):
        kernel = np.ascontiguousarray(kernel, np.float32)
        _check(_lib.mimc3_float_conv2_dev(self._h, d_in, H, W, kernel, kernel.shape[0], kernel.shape[1], d_out, d_scratch, stream),
               "GMA_float_conv2_dev")

    def filter_images(self, kernel):
        """Filter the resident pair on the device and match on the filtered pair from now on; None = back to raw.
        As in the reference program, the output planes are allocated once and a filter never writes their border but reads it (the
        minimum, the shifted right-hand columns): what one filter leaves there is input to the next.  Two filters in a row
        therefore differ from each on its own in the border, and the leftovers can take the pair out of the scaled-integer class
        (negative border values: the f32 kernels then match it, and match_ncc_full_planes refuses it).  filter_images(None) in
        between starts the next filter from fresh planes."""
        if kernel is None:
            _check(_lib.mimc3_ctx_filter_images(self._h, None, 0, 0), "filter_images")
            return
        k = np.ascontiguousarray(kernel, np.float32)
        _check(_lib.mimc3_ctx_filter_images(self._h, k.ctypes.data_as(_vp), k.shape[0], k.shape[1]), "filter_images")

    def get_images(self, H, W):
        i0 = np.empty((H, W), np.float32); i1 = np.empty((H, W), np.float32)
        _check(_lib.mimc3_ctx_get_images(self._h, i0.ctypes.data_as(_vp), i1.ctypes.data_as(_vp)), "get_images")
        return i0, i1

    # -- N1: clustering, dpf0, dpf1 -------------------------------------------------------------
    def calc_mean_var_num_dp_cluster(self, dp, kmax=None):
        """calc_mean_var_num_dp_cluster (MIMC_module.c:994-1130). dp [ndp][N][3] -> (mvn [N][kmax][5], nclus [N]).
        kmax defaults to ndp (always enough); raises Mimc3Error(ECAP) if a point has more clusters than kmax."""
        dp = np.ascontiguousarray(dp, np.float32)
        ndp, n, _ = dp.shape
        kmax = int(kmax or ndp)
        mvn = np.empty((n, kmax, 5), np.float32)
        nclus = np.empty(n, np.int32)
        seen = C.c_int32(0)
        _check(_lib.mimc3_cluster_candidates(self._h, dp, ndp, n, kmax, mvn, nclus, C.byref(seen)),
               "calc_mean_var_num_dp_cluster")
        return mvn, nclus

    def calc_mean_var_num_dp_cluster_dev(self, d_dp, ndp, n, kmax, d_mvn, d_nclus, d_kmax_seen, stream=0):
        _check(_lib.mimc3_cluster_candidates_dev(self._h, d_dp, ndp, n, kmax, d_mvn, d_nclus, d_kmax_seen, stream),
               "calc_mean_var_num_dp_cluster_dev")

    def get_dpf0(self, mvn, nclus, dimx, dimy, min_ratio=0.6):
        """get_dpf0 (MIMC_module.c:1224-1263) -> dpf0 [dimy][dimx]."""
        mvn = np.ascontiguousarray(mvn, np.float32)
        dpf = np.empty(dimx * dimy, np.int32)
        _check(_lib.mimc3_get_dpf0(self._h, mvn, np.ascontiguousarray(nclus, np.int32), dimx * dimy, mvn.shape[1],
                                   min_ratio, dpf), "get_dpf0")
        return dpf.reshape(dimy, dimx)

    def get_dpf0_dev(self, d_mvn, d_nclus, n, kmax, min_ratio, d_dpf, stream=0):
        _check(_lib.mimc3_get_dpf0_dev(self._h, d_mvn, d_nclus, n, kmax, min_ratio, d_dpf, stream), "get_dpf0_dev")

    def get_dpf1(self, dpf0, ruv, mvn, nclus, xyuvav, dt, mpp):
        """get_dpf1 (MIMC_module.c:1330-1718). Returns (dpf1, dx, dy, sweeps); inputs untouched."""
        dimy, dimx = dpf0.shape
        d = np.array(dpf0, np.int32, order="C")
        x = np.empty((dimy, dimx), np.float32)
        y = np.empty((dimy, dimx), np.float32)
        ruv = np.ascontiguousarray(ruv, np.int32)
        mvn = np.ascontiguousarray(mvn, np.float32)
        sw = C.c_int32(0)
        _check(_lib.mimc3_get_dpf1(self._h, dimy, dimx, d.reshape(-1), x.reshape(-1), y.reshape(-1), ruv, ruv.shape[0],
                                   mvn, mvn.shape[1], np.ascontiguousarray(nclus, np.int32),
                                   np.ascontiguousarray(xyuvav, np.float64), dt, mpp, C.byref(sw)), "get_dpf1")
        return d, x, y, sw.value

    def dpf1_workspace_bytes(self, ngrid):
        return int(_lib.mimc3_dpf1_workspace_bytes(ngrid))

    def get_dpf1_dev(self, dimy, dimx, d_dpf, d_dx, d_dy, d_ruv, nn, d_mvn, kmax, d_nclus, d_xyuvav, dt, mpp, d_work,
                     stream=0):
        """Device-resident get_dpf1; synchronises `stream` once per 32 sweeps. Returns the sweep count."""
        sw = C.c_int32(0)
        _check(_lib.mimc3_get_dpf1_dev(self._h, dimy, dimx, d_dpf, d_dx, d_dy, d_ruv, nn, d_mvn, kmax, d_nclus, d_xyuvav,
                                       dt, mpp, d_work, C.byref(sw), stream), "get_dpf1_dev")
        return sw.value

    # -- kernel selection ---------------------------------------------------------------------
    def set_path(self, mode):
        """"auto" (0): u8 kernel when the pair is 8-bit integral, else the tiled f32 kernel, else the general
        one; "general" (1): force the general f32 kernel; "f32" (2): like auto but never the u8 kernel."""
        _check(_lib.mimc3_ctx_set_path(self._h, {"auto": 0, "general": 1, "f32": 2, "u16": 3, "u8px": 4}.get(mode, mode)), "set_path")

    def last_path(self):
        return {0: "general_f32", 1: "u8_exact", 2: "f32_tiled", 3: "u16_scaled", 4: "u8_offset", 5: "u8_mfma", 6: "u8_mfma_full", 7: "u16_full", 8: "f32i_full", 9: "f32g_full", 10: "f32g_wide", 11: "f32g_chip", 12: "u8_mfma_chip", 13: "u16_mfma_chip", 14: "u8_mfma_wide", 15: "u16_mfma_wide", 16: "f32g_wide_chip"}.get(int(_lib.mimc3_ctx_last_path(self._h)), "none")

    # -- timing -------------------------------------------------------------------------------
    def enable_timing(self, on=True):
        _check(_lib.mimc3_ctx_enable_timing(self._h, 1 if on else 0), "enable_timing")

    def last_kernel_ms(self):
        ms = C.c_float(0)
        _check(_lib.mimc3_ctx_last_kernel_ms(self._h, C.byref(ms)), "last_kernel_ms")
        return float(ms.value)
