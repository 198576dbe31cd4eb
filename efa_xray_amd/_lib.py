"""ctypes binding of libefa_hip.so (C ABI declared in include/efa_hip.h).

There is no CPU fallback anywhere in this package: if the shared library is
missing, or no gfx950 device is usable, the calls below raise.
"""
import ctypes
import os
import sys
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libefa_hip.so")

EFA_OK = 0
EFA_ERR_INVALID = -1
EFA_ERR_NO_DEVICE = -2
EFA_ERR_HIP = -3
EFA_ERR_UNSUPPORTED = -4
EFA_ERR_ALLOC = -5

LOC_NONE = 0
LOC_GC = 1

PATH_AUTO = 0
PATH_SWEEP = 1
PATH_TRANSFORM = 2

RELAX_NONE = 0
RELAX_RTPP = 1
RELAX_RTPS = 2

c_double_p = ctypes.POINTER(ctypes.c_double)
c_uint8_p = ctypes.POINTER(ctypes.c_uint8)
c_int64_p = ctypes.POINTER(ctypes.c_int64)
c_int32_p = ctypes.POINTER(ctypes.c_int32)
c_long_p = ctypes.POINTER(ctypes.c_long)
c_void_pp = ctypes.POINTER(ctypes.c_void_p)

# every exported symbol with its (restype, argtypes); tests check this table
# against include/efa_hip.h and against the built library.
SIGNATURES = {
    "efa_abi_version": (ctypes.c_int, []),
    "efa_last_error": (ctypes.c_char_p, []),
    "efa_device_count": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    "efa_ctx_create": (ctypes.c_int, [ctypes.c_int, c_void_pp]),
    "efa_ctx_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "efa_ctx_set_stream": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "efa_ctx_set_option": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_long]),
    "efa_ctx_get_option": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_long)]),
    "efa_ctx_set_relaxation": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_double]),
    "efa_inflate_rows_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "efa_ctx_set_adaptive_inflation": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_double,
                                                      ctypes.c_double, ctypes.c_double]),
    "efa_ctx_set_letkf_inflation": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long,
                                                   ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_void_p]),
    "efa_ctx_set_letkf_control": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p,
                                                 ctypes.c_void_p, ctypes.c_long]),
    "efa_ctx_set_letkf_obs_cap": (ctypes.c_int, [ctypes.c_void_p, c_int32_p, ctypes.c_long, c_long_p, ctypes.c_int, ctypes.c_void_p,
                                                 ctypes.c_long]),
    "efa_ctx_set_letkf_cross_validation": (ctypes.c_int, [ctypes.c_void_p, c_int32_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                          ctypes.c_long]),
    "efa_ctx_set_vertical_localization": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, c_double_p, ctypes.c_long,
                                                         c_double_p, c_double_p]),
    "efa_ctx_set_slab_localization": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, c_double_p, c_int32_p, ctypes.c_long,
                                                     ctypes.c_long, c_double_p, c_double_p, c_int32_p, c_int32_p, ctypes.c_long,
                                                     c_double_p]),
    "efa_slab_factor_table": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_long, c_double_p]),
    "efa_ctx_set_outlier_threshold": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double]),
    "efa_ctx_set_sampling_error_correction": (ctypes.c_int, [ctypes.c_void_p, c_double_p, ctypes.c_int]),
    "efa_etkf_solution": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_double_p, c_double_p, c_double_p, c_double_p,
                                         ctypes.POINTER(ctypes.c_long)]),
    "efa_ctx_synchronize": (ctypes.c_int, [ctypes.c_void_p]),
    "efa_malloc": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, c_void_pp]),
    "efa_free": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "efa_memcpy_h2d": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]),
    "efa_memcpy_d2h": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]),
    "efa_memcpy_d2d": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]),
    "efa_form_perts_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p,
                                          ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]),
    "efa_posterior_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_void_p]),
    "efa_forward_stencil_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_long, ctypes.c_int,
                                               ctypes.c_void_p, ctypes.c_long, ctypes.c_int, c_int64_p,
                                               c_double_p, ctypes.c_void_p]),
    "efa_interp_stencils": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_long, c_double_p, c_double_p, c_double_p, ctypes.c_long,
                                           ctypes.POINTER(ctypes.c_int32), c_double_p, c_double_p, c_double_p,
                                           c_int64_p, c_double_p, c_uint8_p]),
    "efa_forward_interp_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_long,
                                              ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "efa_ensrf_update_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_long,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                            c_double_p, c_double_p, c_uint8_p, ctypes.c_int,
                                            c_double_p, c_double_p, c_double_p, c_double_p, c_double_p,
                                            ctypes.c_long, ctypes.c_long,
                                            c_double_p, c_double_p, c_double_p, c_double_p, c_uint8_p]),
    "efa_obs_phase_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_void_p,
                                         ctypes.c_void_p, c_double_p, c_double_p, c_uint8_p, ctypes.c_int,
                                         c_double_p, c_double_p, c_double_p,
                                         c_double_p, c_double_p, c_double_p, c_double_p, c_uint8_p]),
    "efa_state_phase_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           c_double_p, c_double_p, ctypes.c_long, ctypes.c_long]),
    "efa_state_cycle_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p,
                                           ctypes.c_void_p, c_double_p, c_double_p, ctypes.c_long,
                                           ctypes.c_long]),
    "efa_ensrf_cycle_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_long,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                           c_double_p, c_double_p, c_uint8_p, ctypes.c_int,
                                           c_double_p, c_double_p, c_double_p, c_double_p, c_double_p,
                                           ctypes.c_long, ctypes.c_long,
                                           c_double_p, c_double_p, c_double_p, c_double_p, c_uint8_p]),
    "efa_ensrf_cycle_host": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_void_pp, c_void_pp, ctypes.POINTER(ctypes.c_long),
                                            ctypes.c_long, ctypes.c_int, ctypes.c_long, c_double_p, ctypes.c_long,
                                            c_double_p, c_double_p, c_uint8_p, ctypes.c_int,
                                            c_double_p, c_double_p, c_double_p, c_double_p, c_double_p,
                                            c_double_p, c_double_p, c_double_p, c_double_p, c_uint8_p]),
    "efa_ensrf_cycle_host_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, c_void_pp, c_void_pp, ctypes.POINTER(ctypes.c_long),
                                                ctypes.c_long, ctypes.c_int, ctypes.c_long, c_double_p, ctypes.c_long,
                                                c_double_p, c_double_p, c_uint8_p, ctypes.c_int,
                                                c_double_p, c_double_p, c_double_p, c_double_p, c_double_p,
                                                c_double_p, c_double_p, c_double_p, c_double_p, c_uint8_p]),
    "efa_state_cycle_f32_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p,
                                               ctypes.c_void_p, c_double_p, c_double_p, ctypes.c_long,
                                               ctypes.c_long]),
    "efa_pinned_alloc": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, c_void_pp]),
    "efa_pinned_free": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "efa_ensrf_update": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_long, ctypes.c_int,
                                        ctypes.c_long, c_double_p, c_double_p,
                                        c_double_p, c_double_p, c_uint8_p, ctypes.c_int,
                                        c_double_p, c_double_p, c_double_p, c_double_p, c_double_p,
                                        ctypes.c_long, ctypes.c_long,
                                        c_double_p, c_double_p, c_double_p, c_double_p, c_uint8_p]),
    "efa_cov_contract_f32_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_long,
                                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "efa_obs_impact_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_long,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          c_double_p, c_double_p, c_uint8_p, ctypes.c_int,
                                          c_double_p, c_double_p, c_double_p, c_double_p, c_double_p,
                                          ctypes.c_long, ctypes.c_long, c_double_p]),
    "efa_obs_impact_slab_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_long,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                               c_double_p, c_double_p, c_uint8_p, ctypes.c_int,
                                               c_double_p, c_double_p, c_double_p, c_double_p, c_double_p,
                                               ctypes.c_long, ctypes.c_long, c_double_p]),
    "efa_sensitivity_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, c_double_p,
                                           ctypes.c_long, ctypes.c_long, c_double_p, c_double_p, ctypes.c_void_p, ctypes.c_int,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.POINTER(ctypes.c_long), c_double_p, c_double_p]),
    "efa_sensitivity_f32_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, c_double_p,
                                               ctypes.c_long, ctypes.c_long, c_double_p, c_double_p, ctypes.c_void_p, ctypes.c_int,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.POINTER(ctypes.c_long), c_double_p, c_double_p]),
    "efa_verify_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_long,
                                      ctypes.POINTER(ctypes.c_int), ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong),
                                      ctypes.POINTER(ctypes.c_longlong), c_double_p]),
    "efa_verify_f32_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_long,
                                          ctypes.POINTER(ctypes.c_int), ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong),
                                          ctypes.POINTER(ctypes.c_longlong), c_double_p]),
    "efa_products_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p, ctypes.c_long, ctypes.c_long,
                                        ctypes.c_int, c_double_p, ctypes.c_int, c_double_p, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int),
                                        ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong),
                                        c_double_p]),
    "efa_products_f32_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p, ctypes.c_long,
                                            ctypes.c_long, ctypes.c_int, c_double_p, ctypes.c_int, c_double_p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.POINTER(ctypes.c_int), ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong),
                                            ctypes.POINTER(ctypes.c_longlong), c_double_p]),
    "efa_gram_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p, ctypes.c_long, ctypes.c_long,
                                    c_double_p, ctypes.c_void_p, c_double_p, ctypes.POINTER(ctypes.c_longlong),
                                    ctypes.POINTER(ctypes.c_longlong), c_double_p]),
    "efa_gram_f32_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p, ctypes.c_long, ctypes.c_long,
                                        c_double_p, ctypes.c_void_p, c_double_p, ctypes.POINTER(ctypes.c_longlong),
                                        ctypes.POINTER(ctypes.c_longlong), c_double_p]),
    "efa_neighbourhood_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p, ctypes.c_long,
                                             ctypes.c_long, ctypes.c_long, ctypes.c_int, c_double_p, ctypes.c_int,
                                             ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_void_p,
                                             c_double_p, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]),
    "efa_neighbourhood_f32_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p, ctypes.c_long,
                                                 ctypes.c_long, ctypes.c_long, ctypes.c_int, c_double_p, ctypes.c_int,
                                                 ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_void_p,
                                                 c_double_p, ctypes.POINTER(ctypes.c_longlong),
                                                 ctypes.POINTER(ctypes.c_longlong)]),
    "efa_pm_mean_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p, ctypes.c_long, ctypes.c_long,
                                       ctypes.c_long, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_long, ctypes.c_long,
                                       ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong)]),
    "efa_pm_mean_f32_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p, ctypes.c_long,
                                           ctypes.c_long, ctypes.c_long, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_long,
                                           ctypes.c_long, ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong)]),
    "efa_letkf_cycle_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_long,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                           c_double_p, c_double_p, c_uint8_p,
                                           c_double_p, c_double_p, c_double_p, c_double_p, c_double_p,
                                           ctypes.c_long, ctypes.c_long,
                                           c_double_p, c_double_p, c_double_p, c_double_p, c_uint8_p, ctypes.c_void_p]),
    "efa_letkf_cycle_f32_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_long,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                               c_double_p, c_double_p, c_uint8_p,
                                               c_double_p, c_double_p, c_double_p, c_double_p, c_double_p,
                                               ctypes.c_long, ctypes.c_long,
                                               c_double_p, c_double_p, c_double_p, c_double_p, c_uint8_p, ctypes.c_void_p]),
    "efa_letkf_weights_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p,
                                             c_double_p, c_double_p, c_uint8_p, c_double_p, c_double_p, c_double_p,
                                             ctypes.c_long, c_double_p, c_double_p, ctypes.c_void_p, ctypes.c_void_p]),
    "efa_letkf_cycle_interp_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_long,
                                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                                  c_double_p, c_double_p, c_uint8_p,
                                                  c_double_p, c_double_p, c_double_p, c_double_p, c_double_p,
                                                  ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_long,
                                                  c_double_p, c_double_p, c_double_p, c_double_p, c_uint8_p, ctypes.c_void_p]),
    "efa_letkf_cycle_interp_f32_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_long,
                                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                                      c_double_p, c_double_p, c_uint8_p,
                                                      c_double_p, c_double_p, c_double_p, c_double_p, c_double_p,
                                                      ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_long,
                                                      c_double_p, c_double_p, c_double_p, c_double_p, c_uint8_p, ctypes.c_void_p]),
    "efa_letkf_interp_apply_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_long,
                                                  ctypes.c_void_p, ctypes.c_void_p]),
    "efa_letkf_interp_apply_f32_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                      ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_long, ctypes.c_long,
                                                      ctypes.c_void_p, ctypes.c_void_p]),
    "efa_letkf_slab_groups": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, c_int32_p, ctypes.POINTER(ctypes.c_int)]),
    "efa_last_timing": (ctypes.c_int, [ctypes.c_void_p, c_double_p, c_double_p,
                                       ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_int)]),
    "efa_fill_synthetic_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_long, ctypes.c_int,
                                              ctypes.c_uint64, ctypes.c_double, ctypes.c_void_p]),
    "efa_comm_unique_id": (ctypes.c_int, [c_uint8_p]),
    "efa_comm_init": (ctypes.c_int, [ctypes.c_void_p, c_uint8_p, ctypes.c_int, ctypes.c_int]),
    "efa_comm_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "efa_allreduce_sum_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long]),
    "efa_gc_block_counts": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, c_double_p, c_double_p, ctypes.c_long,
                                           c_double_p, c_double_p, c_double_p, c_uint8_p,
                                           ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                           ctypes.POINTER(ctypes.c_uint64)]),
}

COMM_ID_BYTES = 128


class EfaError(RuntimeError):
    """A libefa_hip call failed (status < 0); message from efa_last_error()."""

    def __init__(self, status, message):
        RuntimeError.__init__(self, "libefa_hip error %d: %s" % (status, message))
        self.status = status


_lib = None


def load_library(path=None):
    """dlopen libefa_hip.so (once) and declare every prototype.

    Raises RuntimeError if the library has not been built -- build it with
    `python -c "import __graft_entry__ as g; g.build()"` or
    `make -C efa_xray_amd/csrc`.  Nothing falls back to a CPU path.
    """
    global _lib
    if _lib is not None and path is None:
        return _lib
    # One HIP runtime per process: the PyTorch wheel bundles its own libamdhip64; if libefa_hip.so pulls in
    # /opt/rocm's copy first and torch is imported later, torch's copy finds no GPU ("No HIP GPUs are
    # available").  Where torch is installed (HipEngine / bench.py use it for device memory and RCCL) it is
    # therefore imported first, so that both resolve to the copy already loaded.
    if "torch" not in sys.modules:
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    # EFA_HIP_LIB: a diagnostic build of the same library (tools/ only; `make -C efa_xray_amd/csrc diag`)
    p = path or os.environ.get("EFA_HIP_LIB") or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError(
            "libefa_hip.so not found at %s: the HIP extension is not built "
            "(run `make -C %s`); efa_xray_amd has no CPU fallback" % (p, os.path.join(_HERE, "csrc")))
    lib = ctypes.CDLL(p)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if a symbol is missing
        fn.restype = res
        fn.argtypes = args
    if lib.efa_abi_version() != 1:
        raise RuntimeError("libefa_hip ABI version %d, expected 1" % lib.efa_abi_version())
    if path is None:
        _lib = lib
    return lib


def _check(lib, status):
    if status != EFA_OK:
        msg = lib.efa_last_error()
        raise EfaError(status, msg.decode("utf-8", "replace") if msg else "")


def device_count():
    lib = load_library()
    n = ctypes.c_int(0)
    _check(lib, lib.efa_device_count(ctypes.byref(n)))
    return n.value


def _dp(a):
    """double* view of a C-contiguous float64 ndarray (or NULL)."""
    if a is None:
        return None
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(c_double_p)


def _llp(a):
    """long long* view of a C-contiguous int64 ndarray."""
    assert a.dtype == np.int64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))


def _u8p(a):
    if a is None:
        return None
    assert a.dtype == np.uint8 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(c_uint8_p)


def state_dtype(dtype):
    """The storage dtype of a state: None -> float64 (the default everywhere); float64 and float32 as given; anything else raises
    ValueError.  float32 is storage only: every number is computed in float64."""
    if dtype is None:
        return np.dtype(np.float64)
    try:
        dt = np.dtype(dtype)
    except TypeError:
        raise ValueError("dtype=%r: expected None, numpy.float64 or numpy.float32" % (dtype,))
    if dt not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise ValueError("dtype=%r: a state is stored as float64 (None) or float32" % (dtype,))
    return dt


def plan_chunks(ncol, chunk_cols, itemsize=8):
    """The column chunks [(lo, hi), ...] of a streamed update (efa_ensrf_cycle_host / _f32): contiguous, covering [0, ncol), every
    cut on a multiple of 16 columns (the one-pass sweep's block), the last chunk taking the ragged rest.  A budget below one block
    gives one block per chunk.  The cuts are in columns, so they are the same for either item size (8 or 4 bytes)."""
    if itemsize not in (4, 8):
        raise ValueError("plan_chunks: itemsize must be 8 (float64) or 4 (float32), got %r" % (itemsize,))
    ncol, chunk_cols = int(ncol), int(chunk_cols)
    if ncol < 0 or chunk_cols < 1:
        raise ValueError("plan_chunks: need ncol >= 0 and chunk_cols >= 1, got %d and %d" % (ncol, chunk_cols))
    cc = max(16, chunk_cols // 16 * 16)
    return [(lo, min(lo + cc, ncol)) for lo in range(0, ncol, cc)]


def default_chunk_cols(n_lead, M, target_bytes=64 << 20, itemsize=8):
    """Columns per chunk for a chunk of about `target_bytes` (n_lead slabs of M members of `itemsize` bytes per column)."""
    if itemsize not in (4, 8):
        raise ValueError("default_chunk_cols: itemsize must be 8 (float64) or 4 (float32), got %r" % (itemsize,))
    return max(16, int(target_bytes // max(1, int(n_lead) * int(M) * int(itemsize))) // 16 * 16)


def compact_stencil(idx):
    """(rows, cidx) for a stencil `idx` of global state rows (any shape, -1 unused): `rows` the distinct rows it names, ascending,
    and `cidx` the same stencil with every entry replaced by its position in `rows` (-1 stays -1).  Applying `cidx` to the
    gathered rows X[rows] is applying `idx` to X, entry by entry in the same order."""
    idx = np.asarray(idx, dtype=np.int64)
    used = idx >= 0
    rows = np.unique(idx[used])
    cidx = np.full(idx.shape, -1, dtype=np.int64)
    cidx[used] = np.searchsorted(rows, idx[used])
    return rows, cidx


class PinnedBlock(object):
    """One block of efa_pinned_alloc, exposed through the array interface: `np.asarray(block)` is a writable view (float64, or the
    block's `dtype`) whose base keeps the block alive; the block goes back to its context's pool when the last view is collected."""

    def __init__(self, ctx, nbytes, dtype=np.float64):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        self.dtype = np.dtype(dtype)
        self.ptr = ctx._pinned_take(self.nbytes)

    @property
    def __array_interface__(self):
        return {"shape": (self.nbytes // self.dtype.itemsize,), "typestr": self.dtype.str, "data": (self.ptr, False), "version": 3}

    def __del__(self):
        try:
            if self.ptr:
                self.ctx._pinned_give(self.ptr, self.nbytes)
            self.ptr = None
        except Exception:
            pass


class DeviceArray(object):
    """A float64 (or, with dtype=numpy.float32, float32) array in the context GPU's HBM (hipMalloc via efa_malloc)."""

    def __init__(self, ctx, shape, dtype=None):
        self.ctx = ctx
        self.shape = tuple(int(s) for s in np.atleast_1d(shape))
        self.dtype = state_dtype(dtype)
        self.itemsize = self.dtype.itemsize
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.itemsize
        ptr = ctypes.c_void_p()
        _check(ctx.lib, ctx.lib.efa_malloc(ctx.handle, self.nbytes, ctypes.byref(ptr)))
        self.ptr = ptr

    @property
    def address(self):
        return self.ptr.value

    def upload(self, host):
        host = np.ascontiguousarray(host, dtype=self.dtype)
        assert host.nbytes == self.nbytes, (host.shape, self.shape)
        _check(self.ctx.lib, self.ctx.lib.efa_memcpy_h2d(self.ctx.handle, self.ptr, host.ctypes.data, self.nbytes))
        return self

    def download(self, out=None):
        if out is None:
            out = np.empty(self.shape, dtype=self.dtype)
        assert out.dtype == self.dtype and out.nbytes == self.nbytes and out.flags["C_CONTIGUOUS"]
        _check(self.ctx.lib, self.ctx.lib.efa_memcpy_d2h(self.ctx.handle, out.ctypes.data, self.ptr, self.nbytes))
        return out

    def upload_rows(self, r0, host):
        """Rows [r0, r0 + len(host)) from a C-contiguous host array of the array's dtype, straight from the caller's memory."""
        host = np.ascontiguousarray(host, dtype=self.dtype)
        width = int(np.prod(self.shape[1:], dtype=np.int64)) if len(self.shape) > 1 else 1
        assert host.size % width == 0 and r0 * width * self.itemsize + host.nbytes <= self.nbytes
        dst = ctypes.c_void_p(self.ptr.value + r0 * width * self.itemsize)
        _check(self.ctx.lib, self.ctx.lib.efa_memcpy_h2d(self.ctx.handle, dst, host.ctypes.data, host.nbytes))

    def download_rows_into(self, r0, out):
        """Rows [r0, r0 + out.size / width) into `out` (C-contiguous, the array's dtype), without an intermediate array."""
        assert out.dtype == self.dtype and out.flags["C_CONTIGUOUS"]
        width = int(np.prod(self.shape[1:], dtype=np.int64)) if len(self.shape) > 1 else 1
        assert out.size % width == 0 and r0 * width * self.itemsize + out.nbytes <= self.nbytes
        src = ctypes.c_void_p(self.ptr.value + r0 * width * self.itemsize)
        _check(self.ctx.lib, self.ctx.lib.efa_memcpy_d2h(self.ctx.handle, out.ctypes.data, src, out.nbytes))
        return out

    def download_rows(self, r0, r1):
        """Rows [r0, r1) of a 2-D (or 1-D) array, without copying the rest."""
        width = int(np.prod(self.shape[1:], dtype=np.int64)) if len(self.shape) > 1 else 1
        out = np.empty((r1 - r0,) + self.shape[1:], dtype=self.dtype)
        src = ctypes.c_void_p(self.ptr.value + r0 * width * self.itemsize)
        _check(self.ctx.lib, self.ctx.lib.efa_memcpy_d2h(self.ctx.handle, out.ctypes.data, src, out.nbytes))
        return out

    def free(self):
        if self.ptr is not None and self.ptr.value and self.ctx.handle is not None:
            self.ctx.lib.efa_free(self.ctx.handle, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# the slab calls of DESIGN.md 7y-3 take the arguments of the calls they stand beside
for _name in ("cycle_dev", "cycle_f32_dev", "cycle_interp_dev", "cycle_interp_f32_dev", "weights_dev"):
    SIGNATURES["efa_letkf_slab_" + _name] = SIGNATURES["efa_letkf_" + _name]
del _name


def letkf_mesh_nodes(n, stride):
    """Node indices of the LETKF's weight-interpolation mesh on an axis of n points: 0, s, 2s, .. below n-1,
    and n-1 itself; one node if n == 1."""
    n, stride = int(n), int(stride)
    if n < 1 or stride < 1:
        raise ValueError("letkf_mesh_nodes: n=%d and stride=%d must be >= 1" % (n, stride))
    if n == 1:
        return np.zeros(1, dtype=np.int64)
    return np.append(np.arange(0, n - 1, stride, dtype=np.int64), n - 1)


class Context(object):
    """One efa_ctx: a GPU, its stream and its workspaces."""

    def __init__(self, device=0):
        self.lib = load_library()
        self.handle = None
        h = ctypes.c_void_p()
        _check(self.lib, self.lib.efa_ctx_create(int(device), ctypes.byref(h)))
        self.handle = h
        self.device = int(device)
        self._pinned_lock = threading.RLock()   # a block may be collected, and given back, on any thread
        self._pinned_pool = {}       # nbytes -> [host addresses] of blocks no array uses any more
        self._pinned_pooled = 0      # bytes in the pool
        self.pinned_live = 0         # bytes of efa_pinned_alloc blocks, pooled ones included
        self.pinned_pool_limit = 4096 << 20

    def close(self):
        """Destroys the context; blocks of `pinned_empty` still alive are freed with it (their arrays must not be used after)."""
        if self.handle is not None:
            self.lib.efa_ctx_destroy(self.handle)
            self.handle = None
            self._pinned_pool, self._pinned_pooled, self.pinned_live = {}, 0, 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- options ------------------------------------------------------------
    def set_option(self, key, value):
        _check(self.lib, self.lib.efa_ctx_set_option(self.handle, key.encode(), int(value)))

    def get_option(self, key):
        v = ctypes.c_long(0)
        _check(self.lib, self.lib.efa_ctx_get_option(self.handle, key.encode(), ctypes.byref(v)))
        return v.value

    def set_relaxation(self, kind, alpha=0.0):
        """Posterior relaxation of every later state phase on this context (RELAX_NONE / RELAX_RTPP / RELAX_RTPS)."""
        _check(self.lib, self.lib.efa_ctx_set_relaxation(self.handle, int(kind), float(alpha)))

    def set_adaptive_inflation(self, field, rows=0, lower=1.0, upper=1e6, sd_lower=0.0):
        """Adaptive inflation (Anderson 2009) of every later GC state phase on this context: `field` a device [rows][2]
        (mean, sd) array updated in place, or None to turn it off."""
        _check(self.lib, self.lib.efa_ctx_set_adaptive_inflation(self.handle, self._addr(field), int(rows), float(lower),
                                                                 float(upper), float(sd_lower)))

    def set_letkf_inflation(self, field, ob_infl=None, P=0, sigma_b=0.0, lower=1e-2, upper=1e2, stats=None):
        """Per-point multiplicative inflation of every later LETKF call on this context (Miyoshi 2011): `field` a
        float64 DeviceArray of one factor per solve point ([ngroups][columns, nodes or probe points]), updated in place when
        sigma_b > 0, or None to turn it off; ob_infl: a DeviceArray [P] of the obs' own factors or None (1.0); stats: a
        DeviceArray [nsolve][4] for {p1, p2, p3, lambda_o} or None."""
        if field is None:
            _check(self.lib, self.lib.efa_ctx_set_letkf_inflation(self.handle, None, 0, None, 0, 0.0, 1.0, 1.0, None))
            return
        _check(self.lib, self.lib.efa_ctx_set_letkf_inflation(self.handle, self._addr(field), int(np.prod(field.shape, dtype=np.int64)),
                                                              self._addr(ob_infl),
                                                              int(P), float(sigma_b), float(lower), float(upper), self._addr(stats)))

    def set_letkf_control(self, xc, xc_post=None, yc=None, yc_post=None):
        """The deterministic control analysis of every later plain or slab LETKF cycle on this context (Schraff et al. 2016;
        DESIGN.md 7y-7): float64 DeviceArrays xc [rows] (the control, one value per state row) and xc_post [rows] (its analysis;
        xc itself for in place), yc [P] (the control's observation estimates H(x_c)) and yc_post [P]; yc and yc_post may be None
        without observations.  xc None turns it off.  The context holds addresses only: keep the arrays alive."""
        if xc is None:
            _check(self.lib, self.lib.efa_ctx_set_letkf_control(self.handle, None, None, 0, None, None, 0))
            return
        rows = int(np.prod(xc.shape, dtype=np.int64))
        P = 0 if yc is None else int(np.prod(yc.shape, dtype=np.int64))
        _check(self.lib, self.lib.efa_ctx_set_letkf_control(self.handle, self._addr(xc), self._addr(xc_post), rows, self._addr(yc),
                                                            self._addr(yc_post), P))

    def set_letkf_obs_cap(self, ob_class, caps, reach=None, P=None):
        """The cap on the local observations of every later plain or weight-interpolated LETKF cycle and of letkf_weights on this
        context: ob_class a host int array [P] of classes 0..len(caps)-1 (None: every ob is of class 0, P then
        gives their number), caps the most obs of each class one local analysis may use, 0 meaning no limit; reach a float64
        DeviceArray [solve points] that receives the count before the cap (kept alive by the caller), or None.  caps None turns
        it off."""
        if caps is None:
            _check(self.lib, self.lib.efa_ctx_set_letkf_obs_cap(self.handle, None, 0, None, 0, None, 0))
            return
        caps_h = np.ascontiguousarray(caps, dtype=np.int64).reshape(-1)
        cls_h = None
        if ob_class is not None:
            cls_h = np.ascontiguousarray(ob_class, dtype=np.int32).reshape(-1)
            if P is not None and int(P) != cls_h.size:
                raise ValueError("set_letkf_obs_cap: ob_class has %d entries, P=%d" % (cls_h.size, int(P)))
            P = cls_h.size
        elif P is None:
            raise ValueError("set_letkf_obs_cap: without ob_class the observation count P must be given")
        nsolve = 0 if reach is None else int(np.prod(reach.shape, dtype=np.int64))
        _check(self.lib, self.lib.efa_ctx_set_letkf_obs_cap(
            self.handle, None if cls_h is None else cls_h.ctypes.data_as(c_int32_p), int(P),
            caps_h.ctypes.data_as(c_long_p), int(caps_h.size), self._addr(reach), nsolve))

    def set_letkf_cross_validation(self, groups, cv_stats=None):
        """The cross-validated perturbation update (Buehner 2020) of every later plain or weight-interpolated LETKF
        cycle and of letkf_weights on this context: groups a host int array [M], the label 0..K-1 of every member (K >= 2, every
        label used, at least 2 members outside every group); cv_stats a float64 DeviceArray [solve points, 2] that receives the
        sub-solves' summed sweeps and largest condition number (kept alive by the caller), or None.  groups None turns it off."""
        if groups is None:
            _check(self.lib, self.lib.efa_ctx_set_letkf_cross_validation(self.handle, None, 0, 0, None, 0))
            return
        g = np.ascontiguousarray(groups, dtype=np.int32).reshape(-1)
        nsolve = 0 if cv_stats is None else int(np.prod(cv_stats.shape, dtype=np.int64)) // 2
        _check(self.lib, self.lib.efa_ctx_set_letkf_cross_validation(
            self.handle, g.ctypes.data_as(c_int32_p), int(g.size), int(g.max()) + 1 if g.size else 0, self._addr(cv_stats), nsolve))

    def set_vertical_localization(self, lead_vert=None, ob_vert=None, ob_vert_halfwidth=None):
        """Vertical localisation of every later GC cycle on this context: host arrays lead_vert [n_lead] and
        ob_vert / ob_vert_halfwidth [P], NaN meaning no vertical taper; lead_vert None turns it off."""
        if lead_vert is None:
            _check(self.lib, self.lib.efa_ctx_set_vertical_localization(self.handle, 0, None, 0, None, None))
            return
        lv = np.ascontiguousarray(lead_vert, dtype=np.float64).reshape(-1)
        ov = np.ascontiguousarray(ob_vert, dtype=np.float64).reshape(-1)
        oh = np.ascontiguousarray(ob_vert_halfwidth, dtype=np.float64).reshape(-1)
        if ov.shape != oh.shape:
            raise ValueError("ob_vert and ob_vert_halfwidth differ in length: %d and %d" % (ov.size, oh.size))
        _check(self.lib, self.lib.efa_ctx_set_vertical_localization(self.handle, lv.size, _dp(lv), ov.size,
                                                                    _dp(ov) if ov.size else None, _dp(oh) if oh.size else None))

    def set_slab_localization(self, n_lead=None, P=0, lead_time=None, ob_time=None, ob_time_halfwidth=None, lead_var=None,
                              ob_group=None, ob_var=None, impact=None):
        """Temporal and cross-variable localisation of every later GC cycle on this context, host arrays:
        lead_time [n_lead] with ob_time / ob_time_halfwidth [P] (NaN: no temporal taper) for the temporal part, lead_var [n_lead]
        with ob_group / ob_var [P] (-1: a row of ones / no target variable) and impact [n_group][n_var] for the variable part;
        a part left None is absent, both absent (or n_lead None) turns the setting off."""
        if n_lead is None or (lead_time is None and impact is None):
            _check(self.lib, self.lib.efa_ctx_set_slab_localization(self.handle, 0, None, None, 0, 0, None, None, None, None, 0, None))
            return
        n_lead, P = int(n_lead), int(P)

        def dbl(a, n, what):
            a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
            if a.size != n:
                raise ValueError("%s has %d values, expected %d" % (what, a.size, n))
            return a

        def i32(a, n, what):
            a = np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
            if a.size != n:
                raise ValueError("%s has %d values, expected %d" % (what, a.size, n))
            return a

        lt = ot = oh = lv = og = ov = C = None
        n_group = n_var = 0
        if lead_time is not None:
            lt, ot, oh = dbl(lead_time, n_lead, "lead_time"), dbl(ob_time, P, "ob_time"), dbl(ob_time_halfwidth, P, "ob_time_halfwidth")
        if impact is not None:
            C = np.ascontiguousarray(impact, dtype=np.float64)
            if C.ndim != 2 or C.size == 0:
                raise ValueError("impact must be a non-empty [n_group][n_var] table, got shape %r" % (C.shape,))
            n_group, n_var = C.shape
            lv, og, ov = i32(lead_var, n_lead, "lead_var"), i32(ob_group, P, "ob_group"), i32(ob_var, P, "ob_var")

        def ip(a):
            return a.ctypes.data_as(c_int32_p) if a is not None and a.size else None

        def dp(a):
            return _dp(a) if a is not None and a.size else None

        _check(self.lib, self.lib.efa_ctx_set_slab_localization(self.handle, n_lead, _dp(lt), ip(lv), n_var, P, dp(ot), dp(oh), ip(og),
                                                                ip(ov), n_group, None if C is None else _dp(C.reshape(-1))))

    def slab_factor_table(self, P, n_lead, download=True):
        """The table S[P][n_lead] of the slab factors (V T) C the one-pass sweep reads while set_slab_localization is on (and
        with it the vertical factor of set_vertical_localization); download False: only brought up to date on the device."""
        out = np.empty((int(P), int(n_lead)), dtype=np.float64) if download else None
        _check(self.lib, self.lib.efa_slab_factor_table(self.handle, int(P), int(n_lead), _dp(out) if out is not None and out.size else None))
        return out

    def set_outlier_threshold(self, threshold=None):
        """Outlier check of every later obs phase on this context: an ob with
        (value - ym)^2 > threshold^2 (var(Yp) + error) is not assimilated; None or 0 turns it off."""
        _check(self.lib, self.lib.efa_ctx_set_outlier_threshold(self.handle, 0.0 if threshold is None else float(threshold)))

    def set_sampling_error_correction(self, alpha=None):
        """Sampling error correction of every later GC cycle on this context: `alpha` a host table of 2..512
        factors, node j at |r| = j/(T-1), read piecewise linearly; None turns it off."""
        if alpha is None:
            _check(self.lib, self.lib.efa_ctx_set_sampling_error_correction(self.handle, None, 0))
            return
        a = np.ascontiguousarray(alpha, dtype=np.float64).reshape(-1)
        if a.size == 0:
            raise ValueError("the sampling error correction table is empty (None turns the correction off)")
        _check(self.lib, self.lib.efa_ctx_set_sampling_error_correction(self.handle, _dp(a), a.size))

    def inflate_rows(self, rows, M, X, field):
        """X[row] <- mean + sqrt(field[row][0]) (X[row] - mean), in place on the device."""
        _check(self.lib, self.lib.efa_inflate_rows_dev(self.handle, rows, M, self._addr(X), self._addr(field)))

    def set_stream(self, hip_stream):
        _check(self.lib, self.lib.efa_ctx_set_stream(self.handle, ctypes.c_void_p(hip_stream or 0)))

    def use_own_stream(self):
        """Back to the context's private non-blocking stream (option "own_stream")."""
        self.set_option("own_stream", 1)

    def synchronize(self):
        _check(self.lib, self.lib.efa_ctx_synchronize(self.handle))

    # -- memory ---------------------------------------------------------------
    def empty(self, shape, dtype=None):
        return DeviceArray(self, shape, dtype)

    def to_device(self, host, dtype=None):
        host = np.ascontiguousarray(host, dtype=state_dtype(dtype))
        return DeviceArray(self, host.shape, host.dtype).upload(host)

    # -- page-locked host memory the context owns (efa_pinned_alloc) ------------
    def _pinned_take(self, nbytes):
        with self._pinned_lock:
            pool = self._pinned_pool.get(nbytes)
            if pool:
                self._pinned_pooled -= nbytes
                return pool.pop()
            ptr = ctypes.c_void_p()
            _check(self.lib, self.lib.efa_pinned_alloc(self.handle, nbytes, ctypes.byref(ptr)))
            self.pinned_live += nbytes
            return ptr.value

    def _pinned_give(self, ptr, nbytes):
        with self._pinned_lock:
            if self.handle is None:      # the context is gone, and the block with it
                return
            if self._pinned_pooled + nbytes <= self.pinned_pool_limit:
                # kept for the next array of this size: page-locking a block costs more than moving its bytes over the link
                self._pinned_pool.setdefault(nbytes, []).append(ptr)
                self._pinned_pooled += nbytes
                return
            self.pinned_live -= nbytes
            self.lib.efa_pinned_free(self.handle, ctypes.c_void_p(ptr))

    def pinned_in_use(self):
        """Bytes of this context's page-locked blocks that arrays still use."""
        return self.pinned_live - self._pinned_pooled

    def pinned_trim(self, keep=()):
        """Free the pooled blocks no array uses, but one block per entry of `keep` (block sizes in bytes) where the pool has it."""
        with self._pinned_lock:
            keep = list(keep)
            pool = {}
            for nbytes, ptrs in self._pinned_pool.items():
                for ptr in ptrs:
                    if nbytes in keep:
                        keep.remove(nbytes)
                        pool.setdefault(nbytes, []).append(ptr)
                        continue
                    self.pinned_live -= nbytes
                    self._pinned_pooled -= nbytes
                    self.lib.efa_pinned_free(self.handle, ctypes.c_void_p(ptr))
            self._pinned_pool = pool

    def pinned_reserve(self, sizes, limit):
        """True if arrays of these sizes (bytes) may be taken from `pinned_empty` with at most `limit` bytes of this context's
        page-locked memory in use afterwards.  Pooled blocks of these sizes are kept for them; other pooled blocks are freed when
        the new blocks would otherwise take the context's total above the limit."""
        with self._pinned_lock:
            sizes = [max(int(n), 8) for n in sizes]
            if self.pinned_in_use() + sum(sizes) > limit:
                return False
            fresh, have = 0, dict((n, len(p)) for n, p in self._pinned_pool.items())
            for n in sizes:
                if have.get(n, 0) > 0:
                    have[n] -= 1
                else:
                    fresh += n
            if self.pinned_live + fresh > limit:
                self.pinned_trim(keep=sizes)
            return True

    def pinned_empty(self, shape, dtype=None):
        """A writable C-contiguous float64 (dtype None) or float32 array in page-locked memory of this context:
        `efa_ensrf_cycle_host` / `_f32` move it by DMA without staging.  The memory goes back to the context when the array (and
        every view of it) is collected."""
        dt = state_dtype(dtype)
        shape = tuple(int(v) for v in np.atleast_1d(shape))
        n = int(np.prod(shape, dtype=np.int64))
        return np.asarray(PinnedBlock(self, max(max(n, 1) * dt.itemsize, 8), dt))[:n].reshape(shape)

    def ensrf_cycle_host(self, seg_prior, seg_post, ncol, M, HX, chunk_cols, ob_value, ob_error, ob_assim, loc_mode=LOC_NONE,
                         ob_lat=None, ob_lon=None, ob_halfwidth=None, grid_lat=None, grid_lon=None):
        """efa_ensrf_cycle_host: one whole cycle on a prior in host memory, streamed through the device in chunks of `chunk_cols`
        columns.  seg_prior / seg_post: lists of C-contiguous float64 arrays (slabs, ncol, M) -- any leading shape that flattens
        to it -- one per variable; the posterior is written into seg_post.  Arrays that are all float32 go through
        efa_ensrf_cycle_host_f32 (float32 storage, float64 arithmetic: DESIGN.md 7g).  Returns the diagnostics."""
        n_seg = len(seg_prior)
        assert len(seg_post) == n_seg
        dts = set(x.dtype for x in list(seg_prior) + list(seg_post))
        if len(dts) > 1:
            raise ValueError("ensrf_cycle_host: the segments mix dtypes %r" % sorted(str(d) for d in dts))
        dt = state_dtype(dts.pop() if dts else None)
        fn = self.lib.efa_ensrf_cycle_host_f32 if dt == np.float32 else self.lib.efa_ensrf_cycle_host
        slabs = (ctypes.c_long * max(n_seg, 1))()
        pin = (ctypes.c_void_p * max(n_seg, 1))()
        pout = (ctypes.c_void_p * max(n_seg, 1))()
        for v, (a, b) in enumerate(zip(seg_prior, seg_post)):
            for x in (a, b):
                assert x.dtype == dt and x.flags["C_CONTIGUOUS"]
            assert a.shape == b.shape and b.flags["WRITEABLE"]
            assert ncol * M == 0 or a.size % (ncol * M) == 0
            slabs[v] = a.size // (ncol * M) if ncol * M else 0
            pin[v] = a.ctypes.data
            pout[v] = b.ctypes.data
        P = 0 if HX is None else int(HX.shape[0])
        if P:
            HX = np.ascontiguousarray(HX, dtype=np.float64)
            assert HX.shape == (P, M)
        val, err, asm, lat, lon, hw = self._ob_arrays(P, ob_value, ob_error, ob_assim, loc_mode, ob_lat, ob_lon, ob_halfwidth)
        glat, glon, gcol = self._grid(loc_mode, grid_lat, grid_lon)
        if loc_mode == LOC_GC:
            assert gcol == ncol
        return self._diagnosed(
            P, fn, self.handle, n_seg, ctypes.cast(pin, c_void_pp), ctypes.cast(pout, c_void_pp), slabs, int(ncol), int(M), P,
            _dp(HX) if P else None, int(chunk_cols), _dp(val), _dp(err), _u8p(asm), loc_mode, _dp(lat), _dp(lon), _dp(hw),
            _dp(glat), _dp(glon))

    def stream_stats(self):
        """The read-only options about the last streamed update."""
        return dict((k, self.get_option("stream_" + k)) for k in ("chunks", "peak_bytes", "h2d_us", "d2h_us", "wall_us"))

    # -- kernels --------------------------------------------------------------
    @staticmethod
    def _addr(x, dtype=np.float64):
        """Device address of `x` for a kernel whose elements are `dtype` (None: any).  A DeviceArray of another dtype raises
        ValueError: a float64 kernel on a float32 allocation would read and write past its end."""
        if x is None:
            return None
        if isinstance(x, DeviceArray):
            if dtype is not None and x.dtype != np.dtype(dtype):
                raise ValueError("this call works on %s device memory, but was given a %s DeviceArray (DESIGN.md 7g)"
                                 % (np.dtype(dtype).name, x.dtype.name))
            return x.ptr
        if isinstance(x, ctypes.c_void_p):
            return x
        return ctypes.c_void_p(int(x))      # raw device address (e.g. torch data_ptr())

    def form_perts(self, rows, M, X, xm, Xp, scale=1.0):
        _check(self.lib, self.lib.efa_form_perts_dev(self.handle, rows, M, self._addr(X), float(scale),
                                                     self._addr(xm), self._addr(Xp)))

    def posterior(self, rows, M, xm, Xp, post):
        _check(self.lib, self.lib.efa_posterior_dev(self.handle, rows, M, self._addr(xm), self._addr(Xp),
                                                    self._addr(post)))

    def forward_stencil(self, rows, row_offset, M, X, idx, wts, HX):
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        wts = np.ascontiguousarray(wts, dtype=np.float64)
        assert idx.ndim == 2 and idx.shape == wts.shape
        P, npt = idx.shape
        _check(self.lib, self.lib.efa_forward_stencil_dev(
            self.handle, rows, row_offset, M, self._addr(X), P, npt,
            idx.ctypes.data_as(c_int64_p), _dp(wts), self._addr(HX)))

    def interp_stencils(self, nvar, nt, ny, nx, grid_lat, grid_lon, valid_times, ob_var, ob_time, ob_lat, ob_lon,
                        want_host=True):
        """f1: build the interpolation stencils of P point obs on the device (they stay in the context for
        `forward_interp`).  Returns (idx (P,8) int64 global rows, wts (P,8), status (P,) uint8) or None."""
        glat = np.ascontiguousarray(grid_lat, dtype=np.float64)
        glon = np.ascontiguousarray(grid_lon, dtype=np.float64)
        latlon_1d = 1 if glat.ndim == 1 else 0
        glat, glon = glat.reshape(-1), glon.reshape(-1)
        vt = np.ascontiguousarray(valid_times, dtype=np.float64).reshape(-1)
        P = len(ob_var)
        var = np.ascontiguousarray(ob_var, dtype=np.int32)
        tim = np.ascontiguousarray(ob_time, dtype=np.float64).reshape(P)
        lat = np.ascontiguousarray(ob_lat, dtype=np.float64).reshape(P)
        lon = np.ascontiguousarray(ob_lon, dtype=np.float64).reshape(P)
        idx = np.full((P, 8), -1, dtype=np.int64)
        wts = np.zeros((P, 8))
        st = np.zeros(P, dtype=np.uint8)
        _check(self.lib, self.lib.efa_interp_stencils(
            self.handle, int(nvar), int(nt), int(ny), int(nx), latlon_1d, glat.shape[0], _dp(glat), _dp(glon), _dp(vt), P,
            var.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _dp(tim), _dp(lat), _dp(lon),
            idx.ctypes.data_as(c_int64_p) if want_host else None, _dp(wts) if want_host else None, _u8p(st)))
        return idx, wts, st

    def forward_interp(self, ncol, col_lo, col_hi, n_lead, M, X, HX):
        _check(self.lib, self.lib.efa_forward_interp_dev(self.handle, ncol, col_lo, col_hi, n_lead, M, self._addr(X),
                                                         self._addr(HX)))

    @staticmethod
    def _ob_arrays(P, ob_value, ob_error, ob_assim, loc_mode, ob_lat, ob_lon, ob_halfwidth):
        val = np.ascontiguousarray(ob_value, dtype=np.float64).reshape(P)
        err = np.ascontiguousarray(ob_error, dtype=np.float64).reshape(P)
        asm = np.ascontiguousarray(np.asarray(ob_assim).astype(bool), dtype=np.uint8).reshape(P)
        lat = lon = hw = None
        if loc_mode == LOC_GC:
            lat = np.ascontiguousarray(ob_lat, dtype=np.float64).reshape(P)
            lon = np.ascontiguousarray(ob_lon, dtype=np.float64).reshape(P)
            hw = np.ascontiguousarray(ob_halfwidth, dtype=np.float64).reshape(P)
        return val, err, asm, lat, lon, hw

    @staticmethod
    def _diag_arrays(P):
        return dict(prior_mean=np.full(P, np.nan), prior_var=np.full(P, np.nan),
                    post_mean=np.full(P, np.nan), post_var=np.full(P, np.nan),
                    assimilated=np.zeros(P, dtype=np.uint8))

    @staticmethod
    def _grid(loc_mode, grid_lat, grid_lon):
        if loc_mode != LOC_GC:
            return None, None, 0
        glat = np.ascontiguousarray(grid_lat, dtype=np.float64).reshape(-1)
        glon = np.ascontiguousarray(grid_lon, dtype=np.float64).reshape(-1)
        assert glat.shape == glon.shape
        return glat, glon, glat.shape[0]

    @classmethod
    def _columns(cls, loc_mode, grid_lat, grid_lon, rows, n_lead):
        """(glat, glon, ncol, n_lead) as the library takes them: the flattened grid and the slabs per column under the GC taper;
        without localisation every row is its own column.  loc_mode None: GC when a grid is given."""
        if loc_mode is None:
            loc_mode = LOC_GC if grid_lat is not None else LOC_NONE
        glat, glon, ncol = cls._grid(loc_mode, grid_lat, grid_lon)
        if loc_mode == LOC_NONE:
            ncol, n_lead = rows, 1
        return glat, glon, ncol, n_lead

    def _diagnosed(self, P, entry, *args, tail=()):
        """entry(*args, <the five diagnostics>, *tail) on fresh diagnostics [P]; returns them as a dict, `assimilated` as bool."""
        d = self._diag_arrays(P)
        _check(self.lib, entry(*(args + (_dp(d["prior_mean"]), _dp(d["prior_var"]), _dp(d["post_mean"]), _dp(d["post_var"]),
                                         _u8p(d["assimilated"])) + tail)))
        d["assimilated"] = d["assimilated"].astype(bool)
        return d

    def obs_phase(self, M, P, ym, Yp, ob_value, ob_error, ob_assim, loc_mode=LOC_NONE,
                  ob_lat=None, ob_lon=None, ob_halfwidth=None):
        """Phase A.  Returns the per-ob diagnostics dict."""
        val, err, asm, lat, lon, hw = self._ob_arrays(P, ob_value, ob_error, ob_assim, loc_mode,
                                                      ob_lat, ob_lon, ob_halfwidth)
        return self._diagnosed(P, self.lib.efa_obs_phase_dev, self.handle, M, P, self._addr(ym), self._addr(Yp), _dp(val), _dp(err),
                               _u8p(asm), loc_mode, _dp(lat), _dp(lon), _dp(hw))

    def etkf_solution(self, M):
        """efa_etkf_solution: the batch solve of the last obs phase, which must have run with option "obs_solver" 1,
        as a dict: T (M, M), w (M,), eigenvalues (M,) of C descending, n_active, q, dfs, chi2, sweeps."""
        M = int(M)
        T = np.empty((max(M, 0), max(M, 0)))
        w = np.empty(max(M, 0))
        eig = np.empty(max(M, 0))
        stats = np.zeros(4)
        sweeps = ctypes.c_long(0)
        _check(self.lib, self.lib.efa_etkf_solution(self.handle, M, _dp(T), _dp(w), _dp(eig), _dp(stats), ctypes.byref(sweeps)))
        return dict(T=T, w=w, eigenvalues=eig, n_active=int(stats[0]), q=float(stats[1]), dfs=float(stats[2]),
                    chi2=float(stats[3]), sweeps=int(sweeps.value))

    def state_phase(self, rows, M, xm_in, Xp_in, xm_out, Xp_out, grid_lat=None, grid_lon=None, n_lead=1):
        glat, glon, ncol, n_lead = self._columns(None, grid_lat, grid_lon, rows, n_lead)
        _check(self.lib, self.lib.efa_state_phase_dev(
            self.handle, rows, M, self._addr(xm_in), self._addr(Xp_in), self._addr(xm_out),
            self._addr(Xp_out), _dp(glat), _dp(glon), ncol, n_lead))

    def _state_cycle(self, entry, dtype, rows, M, X, post, grid_lat, grid_lon, n_lead):
        glat, glon, ncol, n_lead = self._columns(None, grid_lat, grid_lon, rows, n_lead)
        _check(self.lib, entry(self.handle, rows, M, self._addr(X, dtype), self._addr(post, dtype), _dp(glat), _dp(glon), ncol, n_lead))

    def state_cycle(self, rows, M, X, post, grid_lat=None, grid_lon=None, n_lead=1):
        self._state_cycle(self.lib.efa_state_cycle_dev, np.float64, rows, M, X, post, grid_lat, grid_lon, n_lead)

    def state_cycle_f32(self, rows, M, X, post, grid_lat=None, grid_lon=None, n_lead=1):
        """efa_state_cycle_f32_dev: `state_cycle` on float32 member rows (posterior = the float64 result rounded once)."""
        self._state_cycle(self.lib.efa_state_cycle_f32_dev, np.float32, rows, M, X, post, grid_lat, grid_lon, n_lead)

    def ensrf_cycle(self, rows, M, P, X, post, ym, Yp, ob_value, ob_error, ob_assim, loc_mode=LOC_NONE,
                    ob_lat=None, ob_lon=None, ob_halfwidth=None, grid_lat=None, grid_lon=None, n_lead=1, obs_block_out=False):
        """Phase A + the state phase on resident prior members in ONE call (efa_ensrf_cycle_dev): Phase B goes into the stream
        behind Phase A without a host round trip when the cycle is unlocalised and takes the transform.  Returns the diagnostics."""
        val, err, asm, lat, lon, hw = self._ob_arrays(P, ob_value, ob_error, ob_assim, loc_mode,
                                                      ob_lat, ob_lon, ob_halfwidth)
        glat, glon, ncol, n_lead = self._columns(loc_mode, grid_lat, grid_lon, rows, n_lead)
        return self._diagnosed(
            P, self.lib.efa_ensrf_cycle_dev, self.handle, rows, M, P, self._addr(X), self._addr(post), self._addr(ym),
            self._addr(Yp), 1 if obs_block_out else 0, _dp(val), _dp(err), _u8p(asm), loc_mode, _dp(lat), _dp(lon), _dp(hw),
            _dp(glat), _dp(glon), ncol, n_lead)

    def letkf_cycle(self, rows, M, P, X, post, ym, Yp, ob_value, ob_error, ob_assim, ob_lat, ob_lon, ob_halfwidth, grid_lat,
                    grid_lon, n_lead=1, obs_block_out=False, col_stats=None, f32=None, shape=None, stride=None, _slab=False):
        """efa_letkf_cycle_dev / _f32_dev: the LETKF on resident prior members, one ensemble-space solve per
        column under the Gaspari-Cohn taper and one per ob position for the obs block.  col_stats: a float64 DeviceArray
        (ncol, 3) for {n_local, dfs, sweeps} of every column, or None.  f32: the rows' storage (None: X's dtype).  Returns the
        diagnostics.
        With shape=(ny, nx) and stride=(s_y, s_x): efa_letkf_cycle_interp_dev / _f32_dev, the solve at the nodes
        of the mesh only and the pairs interpolated to every column; col_stats then takes the NODE statistics, (nnodes, 3) in the
        order of `letkf_mesh_nodes`."""
        val, err, asm, lat, lon, hw = self._ob_arrays(P, ob_value, ob_error, ob_assim, LOC_GC, ob_lat, ob_lon, ob_halfwidth)
        glat, glon, ncol = self._grid(LOC_GC, grid_lat, grid_lon)
        if f32 is None:
            f32 = isinstance(X, DeviceArray) and X.dtype == np.float32
        dt = np.float32 if f32 else np.float64
        head = (self.handle, rows, M, P, self._addr(X, dt), self._addr(post, dt), self._addr(ym), self._addr(Yp),
                1 if obs_block_out else 0, _dp(val), _dp(err), _u8p(asm), _dp(lat), _dp(lon), _dp(hw), _dp(glat), _dp(glon))
        stem = "efa_letkf_slab_cycle_" if _slab else "efa_letkf_cycle_"
        if stride is None:
            entry, cols = getattr(self.lib, stem + ("f32_dev" if f32 else "dev")), (ncol,)
        else:
            if shape is None:
                raise ValueError("letkf_cycle: stride needs the grid's shape=(ny, nx)")
            entry = getattr(self.lib, stem + ("interp_f32_dev" if f32 else "interp_dev"))
            cols = (int(shape[0]), int(shape[1]), int(stride[0]), int(stride[1]))
        return self._diagnosed(P, entry, *(head + cols + (n_lead,)), tail=(self._addr(col_stats),))

    def letkf_slab_cycle(self, rows, M, P, X, post, ym, Yp, ob_value, ob_error, ob_assim, ob_lat, ob_lon, ob_halfwidth, grid_lat,
                         grid_lon, n_lead=1, obs_block_out=False, col_stats=None, f32=None, shape=None, stride=None):
        """efa_letkf_slab_cycle_dev / _f32_dev / _interp_dev / _interp_f32_dev: `letkf_cycle` with one solve per
        (slab group, column) under the context's vertical and / or slab setting, which must be on and sized for P and n_lead.
        col_stats: a float64 DeviceArray (ngroups, ncol, 3), or (ngroups, nnodes, 3) with a stride; ngroups from
        `letkf_slab_groups`."""
        return self.letkf_cycle(rows, M, P, X, post, ym, Yp, ob_value, ob_error, ob_assim, ob_lat, ob_lon, ob_halfwidth, grid_lat,
                                grid_lon, n_lead, obs_block_out, col_stats, f32, shape, stride, _slab=True)

    def letkf_slab_groups(self, n_lead):
        """efa_letkf_slab_groups: (group_of_slab int32 [n_lead], ngroups) under the context's vertical and / or slab setting."""
        g = np.empty(int(n_lead), dtype=np.int32)
        n = ctypes.c_int(0)
        _check(self.lib, self.lib.efa_letkf_slab_groups(self.handle, int(n_lead), g.ctypes.data_as(c_int32_p) if g.size else None,
                                                        ctypes.byref(n)))
        return g, n.value

    def _letkf_weights(self, entry, ngroups, M, P, ym, Yp, ob_value, ob_error, ob_assim, ob_lat, ob_lon, ob_halfwidth, pt_lat, pt_lon):
        """The solve at the given points through `entry`.  Returns the downloaded pairs (ngroups, npts, M, M + 1) and statistics
        (ngroups, npts, 3); ngroups None: the plain entry, one group."""
        val, err, asm, lat, lon, hw = self._ob_arrays(P, ob_value, ob_error, ob_assim, LOC_GC, ob_lat, ob_lon, ob_halfwidth)
        plat = np.ascontiguousarray(pt_lat, dtype=np.float64).reshape(-1)
        plon = np.ascontiguousarray(pt_lon, dtype=np.float64).reshape(-1)
        assert plat.shape == plon.shape
        npts = plat.shape[0]
        ng = 1 if ngroups is None else ngroups
        Tw = self.empty((ng, max(npts, 1), M, M + 1))
        st = self.empty((ng, max(npts, 1), 3))
        _check(self.lib, entry(self.handle, M, P, self._addr(ym), self._addr(Yp), _dp(val), _dp(err), _u8p(asm), _dp(lat), _dp(lon),
                               _dp(hw), npts, _dp(plat), _dp(plon), self._addr(Tw), self._addr(st)))
        return Tw.download()[:, :npts], st.download()[:, :npts]

    def letkf_slab_weights(self, M, P, ym, Yp, ob_value, ob_error, ob_assim, ob_lat, ob_lon, ob_halfwidth, pt_lat, pt_lon, n_lead):
        """efa_letkf_slab_weights_dev: the solve of every slab group at the given points.  Returns (T (ngroups, npts, M, M),
        w (ngroups, npts, M), stats (ngroups, npts, 3))."""
        _, ng = self.letkf_slab_groups(n_lead)
        tw, st = self._letkf_weights(self.lib.efa_letkf_slab_weights_dev, ng, M, P, ym, Yp, ob_value, ob_error, ob_assim, ob_lat,
                                     ob_lon, ob_halfwidth, pt_lat, pt_lon)
        return np.ascontiguousarray(tw[..., :M]), np.ascontiguousarray(tw[..., M]), st

    def letkf_interp_apply(self, rows, M, X, post, shape, stride, n_lead, Tw_nodes, node_stats=None, f32=None):
        """efa_letkf_interp_apply_dev / _f32_dev: the interpolate-and-apply launch alone.  Tw_nodes: a float64
        DeviceArray (nnodes, M, M + 1) of node pairs, row a of a node = T[a][0..M) | w[a], nodes in the order of
        `letkf_mesh_nodes`; node_stats: (nnodes, 3) whose first entry is n_local, or None (every node counts as reached).  The
        context's relaxation applies."""
        if f32 is None:
            f32 = isinstance(X, DeviceArray) and X.dtype == np.float32
        entry = self.lib.efa_letkf_interp_apply_f32_dev if f32 else self.lib.efa_letkf_interp_apply_dev
        dt = np.float32 if f32 else np.float64
        _check(self.lib, entry(self.handle, rows, M, self._addr(X, dt), self._addr(post, dt), int(shape[0]), int(shape[1]),
                               int(stride[0]), int(stride[1]), n_lead, self._addr(Tw_nodes), self._addr(node_stats)))

    def letkf_weights(self, M, P, ym, Yp, ob_value, ob_error, ob_assim, ob_lat, ob_lon, ob_halfwidth, pt_lat, pt_lon):
        """efa_letkf_weights_dev: the LETKF solve at the given points.  Returns (T (npts, M, M), w (npts, M), stats (npts, 3) =
        {n_local, dfs, sweeps})."""
        tw, st = self._letkf_weights(self.lib.efa_letkf_weights_dev, None, M, P, ym, Yp, ob_value, ob_error, ob_assim, ob_lat,
                                     ob_lon, ob_halfwidth, pt_lat, pt_lon)
        return np.ascontiguousarray(tw[0, :, :, :M]), np.ascontiguousarray(tw[0, :, :, M]), st[0]

    def ensrf_update_dev(self, rows, M, P, xm, Xp, ym, Yp, ob_value, ob_error, ob_assim,
                         loc_mode=LOC_NONE, ob_lat=None, ob_lon=None, ob_halfwidth=None,
                         grid_lat=None, grid_lon=None, n_lead=1):
        val, err, asm, lat, lon, hw = self._ob_arrays(P, ob_value, ob_error, ob_assim, loc_mode,
                                                      ob_lat, ob_lon, ob_halfwidth)
        glat, glon, ncol, n_lead = self._columns(loc_mode, grid_lat, grid_lon, rows, n_lead)
        return self._diagnosed(
            P, self.lib.efa_ensrf_update_dev, self.handle, rows, M, P, self._addr(xm), self._addr(Xp), self._addr(ym),
            self._addr(Yp), _dp(val), _dp(err), _u8p(asm), loc_mode, _dp(lat), _dp(lon), _dp(hw), _dp(glat), _dp(glon), ncol, n_lead)

    def ensrf_update_host(self, xbm, Xbp, nstate, ob_value, ob_error, ob_assim, loc_mode=LOC_NONE,
                          ob_lat=None, ob_lon=None, ob_halfwidth=None, grid_lat=None, grid_lon=None,
                          n_lead=1):
        """efa_ensrf_update on the reference's augmented host arrays, in place."""
        assert xbm.dtype == np.float64 and Xbp.dtype == np.float64
        assert xbm.flags["C_CONTIGUOUS"] and Xbp.flags["C_CONTIGUOUS"]
        A, M = Xbp.shape
        P = A - nstate
        val, err, asm, lat, lon, hw = self._ob_arrays(P, ob_value, ob_error, ob_assim, loc_mode,
                                                      ob_lat, ob_lon, ob_halfwidth)
        glat, glon, ncol, n_lead = self._columns(loc_mode, grid_lat, grid_lon, nstate, n_lead)
        return self._diagnosed(
            P, self.lib.efa_ensrf_update, self.handle, A, nstate, M, P, _dp(xbm), _dp(Xbp), _dp(val), _dp(err), _u8p(asm), loc_mode,
            _dp(lat), _dp(lon), _dp(hw), _dp(glat), _dp(glon), ncol, n_lead)

    def obs_impact(self, rows, M, P, Xf, werr, Ya, innov, ob_error, ob_used, loc_mode=LOC_NONE, ob_lat=None, ob_lon=None,
                   ob_halfwidth=None, grid_lat=None, grid_lon=None, n_lead=1):
        """efa_obs_impact_dev: the forecast impact (P,) of every used ob, 0.0 for the others.  Xf (rows, M), werr
        (rows,) and Ya (P, M) are device arrays and are only read; the per-ob arrays and the grid are host arrays."""
        return self._obs_impact(self.lib.efa_obs_impact_dev, rows, M, P, Xf, werr, Ya, innov, ob_error, ob_used, loc_mode, ob_lat,
                                ob_lon, ob_halfwidth, grid_lat, grid_lon, n_lead)

    def obs_impact_slab(self, rows, M, P, Xf, werr, Ya, innov, ob_error, ob_used, loc_mode=LOC_NONE, ob_lat=None, ob_lon=None,
                        ob_halfwidth=None, grid_lat=None, grid_lon=None, n_lead=1):
        """efa_obs_impact_slab_dev: obs_impact under the temporal and variable tapers of set_slab_localization
        (times the vertical factor while set_vertical_localization is on); obs_impact itself while that setting is off."""
        return self._obs_impact(self.lib.efa_obs_impact_slab_dev, rows, M, P, Xf, werr, Ya, innov, ob_error, ob_used, loc_mode,
                                ob_lat, ob_lon, ob_halfwidth, grid_lat, grid_lon, n_lead)

    def _obs_impact(self, entry, rows, M, P, Xf, werr, Ya, innov, ob_error, ob_used, loc_mode, ob_lat, ob_lon, ob_halfwidth, grid_lat,
                    grid_lon, n_lead):
        d, err, used, lat, lon, hw = self._ob_arrays(P, innov, ob_error, ob_used, loc_mode, ob_lat, ob_lon, ob_halfwidth)
        glat, glon, ncol, n_lead = self._columns(loc_mode, grid_lat, grid_lon, rows, n_lead)
        out = np.zeros(P)
        _check(self.lib, entry(
            self.handle, rows, M, P, self._addr(Xf), self._addr(werr), self._addr(Ya), _dp(d), _dp(err), _u8p(used), loc_mode,
            _dp(lat), _dp(lon), _dp(hw), _dp(glat), _dp(glon), ncol, n_lead, _dp(out)))
        return out

    def _elem_entry(self, name, X, f32):
        """(entry point efa_<name>_dev or efa_<name>_f32_dev, the address of X as that element type); f32 None: X's own dtype"""
        if f32 is None:
            f32 = isinstance(X, DeviceArray) and X.dtype == np.float32
        return getattr(self.lib, "efa_%s%s_dev" % (name, "_f32" if f32 else "")), self._addr(X, np.float32 if f32 else np.float64)

    @staticmethod
    def _group_outputs(slab_group, *shapes):
        """slab_group as an int* (which keeps its array alive) and, for G = its largest group + 1, a zeroed int64 array of shape (G,) + s for every s of shapes"""
        sg = np.ascontiguousarray(slab_group, dtype=np.int32).reshape(-1)
        G = int(sg.max()) + 1 if sg.size and sg.max() >= 0 else 0
        return (sg.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), G) + tuple(np.zeros((G,) + s, dtype=np.int64) for s in shapes)

    def sensitivity(self, rows, M, X, J, slab_error, ncol=None, n_lead=1, weights=None, cand=None, n_targets=0, var=None, cov=None,
                    sens=None, corr=None, dvar=None, score=None, f32=None):
        """efa_sensitivity_dev / efa_sensitivity_f32_dev.  X (rows, M) is a device array of float64 or float32
        members (`f32` says which for a raw address; None: the DeviceArray's dtype), only read; J (K, M), slab_error (n_lead,)
        and weights (K,) are host arrays; cand (rows,) uint8 and the fields var (rows,), cov / sens / corr / dvar (K, rows),
        score (rows,) are float64 device arrays or None (field not wanted).  Returns (picked_row (n_targets,) int64,
        picked_score (n_targets,), metric_var (n_targets + 1, K))."""
        J = np.ascontiguousarray(J, dtype=np.float64)
        K = int(J.shape[0])
        R = np.ascontiguousarray(slab_error, dtype=np.float64).reshape(-1)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        fn, X_p = self._elem_entry("sensitivity", X, f32)
        n = int(n_targets)
        prow = np.full(max(n, 0), -1, dtype=np.int64)
        psc = np.zeros(max(n, 0))
        mv = np.zeros((max(n, 0) + 1, max(K, 1)))
        _check(self.lib, fn(
            self.handle, int(rows), int(M), K, X_p, _dp(J),
            int(rows if ncol is None else ncol), int(n_lead), _dp(R), _dp(w), self._addr(cand, None), n,
            self._addr(var), self._addr(cov), self._addr(sens), self._addr(corr), self._addr(dvar), self._addr(score),
            prow.ctypes.data_as(ctypes.POINTER(ctypes.c_long)), _dp(psc), _dp(mv)))
        return prow, psc, mv

    def verify(self, rows, M, X, verif, slab_group, ncol=None, n_lead=1, col_offset=0, ncol_total=None, col_weight=None,
               fair=False, seed=0, below=None, equal=None, rank=None, crps=None, err=None, var=None, groups=True, f32=None):
        """efa_verify_dev / efa_verify_f32_dev.  X (rows, M) is a device array of float64 or float32 members
        (`f32` says which for a raw address; None: the DeviceArray's dtype) and verif (rows,) a float64 device array, both only
        read; slab_group (n_lead,) is a host array of group numbers (-1: slab not verified); col_weight (ncol,) a float64
        device array or None.  The fields below / equal / rank (int32) are raw device addresses (`malloc_bytes`) or None,
        crps / err / var float64 device arrays or None.  Returns (hist (G, M+1), n (G,), n_bad (G,) int64, sums (G, 5)), or
        None with groups=False (fields only)."""
        fn, X_p = self._elem_entry("verify", X, f32)
        ncol = int(rows if ncol is None else ncol)
        sg_p, G, hist, n, n_bad = self._group_outputs(slab_group, (int(M) + 1,), (), ())
        sums = np.zeros((G, 5))
        out = (_llp(hist), _llp(n), _llp(n_bad), _dp(sums)) if groups else (None,) * 4
        _check(self.lib, fn(
            self.handle, int(rows), int(M), X_p, self._addr(verif), ncol,
            int(n_lead), int(col_offset), int(ncol if ncol_total is None else ncol_total),
            sg_p, self._addr(col_weight), 1 if fair else 0,
            ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), self._addr(below, None), self._addr(equal, None),
            self._addr(rank, None), self._addr(crps), self._addr(err), self._addr(var), *out))
        return (hist, n, n_bad, sums) if groups else None

    def products(self, rows, M, X, ncol=None, n_lead=1, quantiles=(), thresholds=None, mean=None, sd=None, quant=None, prob=None,
                 verif=None, slab_group=None, col_weight=None, f32=None):
        """efa_products_dev / efa_products_f32_dev.  X (rows, M) is a device array of float64 or float32 members
        (`f32` says which for a raw address; None: the DeviceArray's dtype), only read; quantiles a host sequence of at most 8
        levels in [0, 1]; thresholds a host array (n_lead, T), T <= 8, NaN where a slab has no threshold.  The fields mean / sd
        (rows,), quant (Q, rows) and prob (T, rows) are float64 device arrays or None.  With verif (rows,), a float64 device
        array, slab_group (n_lead,) is a host array of group numbers (-1: slab not scored) and col_weight (ncol,) a float64
        device array or None; the call then returns (table (G, T, M+1, 2), n_bad (G, T) int64, sums (G, T, 4)), else None."""
        fn, X_p = self._elem_entry("products", X, f32)
        ncol = int(rows if ncol is None else ncol)
        q = np.ascontiguousarray(quantiles, dtype=np.float64).reshape(-1)
        thr = np.zeros((int(n_lead), 0)) if thresholds is None else np.ascontiguousarray(thresholds, dtype=np.float64)
        thr = thr.reshape(int(n_lead), -1) if thr.size else np.zeros((int(n_lead), 0))
        T = thr.shape[1]
        sg_p, out, res = None, (None, None, None), None
        if verif is not None:
            sg_p, G, table, n_bad = self._group_outputs(slab_group, (T, int(M) + 1, 2), (T,))
            sums = np.zeros((G, T, 4))
            out = (_llp(table), _llp(n_bad), _dp(sums))
            res = (table, n_bad, sums)
        _check(self.lib, fn(
            self.handle, int(rows), int(M), X_p, ncol, int(n_lead), int(q.size), _dp(q),
            int(T), _dp(thr), self._addr(mean), self._addr(sd), self._addr(quant), self._addr(prob), self._addr(verif), sg_p,
            self._addr(col_weight), *out))
        return res

    def neighbourhood(self, rows, M, X, ny, nx, n_lead, thresholds, radii, shape=0, wrap_x=False, nep=None, nmep=None, verif=None,
                      slab_group=None, col_weight=None, f32=None):
        """efa_neighbourhood_dev / efa_neighbourhood_f32_dev.  X (rows, M), rows = n_lead*ny*nx, is a device array of
        float64 or float32 members (`f32` says which for a raw address; None: the DeviceArray's dtype), only read; thresholds a
        host array (n_lead, T), 1 <= T <= 8, NaN where a slab has no threshold; radii a host sequence of at most 4 integers in
        [0, 64]; shape 0 (square) or 1 (disc).  The fields nep / nmep (R, T, rows) are float64 device arrays or None.  With verif
        (rows,), a float64 device array, slab_group (n_lead,) is a host array of group numbers (-1: slab not scored) and
        col_weight (ny*nx,) a float64 device array or None; the call then returns (sums (G, R, T, 6), n (G, R, T), n_bad
        (G, R, T) int64), else None."""
        fn, X_p = self._elem_entry("neighbourhood", X, f32)
        thr = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(int(n_lead), -1)
        rad = np.ascontiguousarray(radii, dtype=np.int32).reshape(-1)
        T, R = thr.shape[1], rad.size
        sg_p, out, res = None, (None, None, None), None
        if verif is not None:
            sg_p, G, n, n_bad = self._group_outputs(slab_group, (R, T), (R, T))
            sums = np.zeros((G, R, T, 6))
            out = (_dp(sums), _llp(n), _llp(n_bad))
            res = (sums, n, n_bad)
        _check(self.lib, fn(
            self.handle, int(rows), int(M), X_p, int(ny), int(nx), int(n_lead), int(T),
            _dp(thr), int(R), rad.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), int(shape), 1 if wrap_x else 0, self._addr(nep),
            self._addr(nmep), self._addr(verif), sg_p, self._addr(col_weight), *out))
        return res

    def pm_mean(self, rows, M, X, ny, nx, n_lead, rank, pm, slab_on=None, patch=None, pick=None, f32=None):
        """efa_pm_mean_dev / efa_pm_mean_f32_dev.  X (rows, M), rows = n_lead*ny*nx, is a device array of float64 or
        float32 members (`f32` says which for a raw address; None: the DeviceArray's dtype) and rank (rows,) a float64 device
        array, both only read; pm (rows,) a float64 device array, written for every row; slab_on (n_lead,) a host array (0: the
        slab is not read) or None; patch (py, px) or None (the whole slab); pick an int in [0, M) or None (M // 2).  Returns
        n_bad (n_lead,) int64."""
        fn, X_p = self._elem_entry("pm_mean", X, f32)
        py, px = (int(ny), int(nx)) if patch is None else (int(patch[0]), int(patch[1]))
        on_p = None
        if slab_on is not None:
            on = np.ascontiguousarray(slab_on, dtype=np.int32).reshape(-1)
            if on.size != int(n_lead):
                raise ValueError("slab_on has %d entries, the state %d slabs" % (on.size, int(n_lead)))
            on_p = on.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
        n_bad = np.zeros(int(n_lead), dtype=np.int64)
        _check(self.lib, fn(
            self.handle, int(rows), int(M), X_p, int(ny), int(nx), int(n_lead),
            self._addr(rank), on_p, py, px, int(M) // 2 if pick is None else int(pick), self._addr(pm),
            _llp(n_bad)))
        return n_bad

    def gram(self, rows, M, X, slab_scale, ncol=None, n_lead=1, col_weight=None, f32=None):
        """efa_gram_dev / efa_gram_f32_dev.  X (rows, M) is a device array of float64 or float32 members (`f32`
        says which for a raw address; None: the DeviceArray's dtype), only read; slab_scale (n_lead,) is a host array of scales
        >= 0 (0: the slab is not read); col_weight (ncol,) a float64 device array or None.  Returns (gram (M, M), n, n_bad,
        sums (2,) = sum w, sum w s^2) over the used, good rows."""
        sc = np.ascontiguousarray(slab_scale, dtype=np.float64).reshape(-1)
        fn, X_p = self._elem_entry("gram", X, f32)
        G = np.zeros((int(M), int(M)))
        n, n_bad = ctypes.c_longlong(0), ctypes.c_longlong(0)
        sums = np.zeros(2)
        _check(self.lib, fn(
            self.handle, int(rows), int(M), X_p, int(rows if ncol is None else ncol),
            int(n_lead), _dp(sc), self._addr(col_weight), _dp(G), ctypes.byref(n), ctypes.byref(n_bad), _dp(sums)))
        return G, int(n.value), int(n_bad.value), sums

    def cov_contract_f32(self, N, M, P, Xbp_f32, Ye_f32, C_f32):
        """C (N x P) = Xbp (N x M) . Ye^T (P x M), float32, device addresses."""
        _check(self.lib, self.lib.efa_cov_contract_f32_dev(self.handle, N, M, P, self._addr(Xbp_f32, np.float32),
                                                           self._addr(Ye_f32, np.float32), self._addr(C_f32, np.float32)))

    def malloc_bytes(self, nbytes):
        ptr = ctypes.c_void_p()
        _check(self.lib, self.lib.efa_malloc(self.handle, int(nbytes), ctypes.byref(ptr)))
        return ptr

    def free_bytes(self, ptr):
        _check(self.lib, self.lib.efa_free(self.handle, ptr))

    def h2d(self, dst_ptr, host):
        host = np.ascontiguousarray(host)
        _check(self.lib, self.lib.efa_memcpy_h2d(self.handle, dst_ptr, host.ctypes.data, host.nbytes))

    def d2h(self, host_out, src_ptr):
        assert host_out.flags["C_CONTIGUOUS"]
        _check(self.lib, self.lib.efa_memcpy_d2h(self.handle, host_out.ctypes.data, src_ptr, host_out.nbytes))

    def last_timing(self):
        s = ctypes.c_double(0)
        o = ctypes.c_double(0)
        n = ctypes.c_long(0)
        p = ctypes.c_int(0)
        _check(self.lib, self.lib.efa_last_timing(self.handle, ctypes.byref(s), ctypes.byref(o),
                                                  ctypes.byref(n), ctypes.byref(p)))
        return dict(state_ms=s.value, obs_ms=o.value, state_launches=n.value, path=p.value)

    # -- multi-GPU: the communicator the context owns (RCCL) -----------------------------------------
    def comm_unique_id(self):
        """A fresh RCCL id (bytes) for rank 0 to hand to the other ranks."""
        buf = np.zeros(COMM_ID_BYTES, dtype=np.uint8)
        _check(self.lib, self.lib.efa_comm_unique_id(_u8p(buf)))
        return buf.tobytes()

    def comm_init(self, comm_id, rank, world):
        buf = np.frombuffer(bytes(comm_id), dtype=np.uint8).copy()
        assert buf.size == COMM_ID_BYTES
        _check(self.lib, self.lib.efa_comm_init(self.handle, _u8p(buf), int(rank), int(world)))

    def comm_destroy(self):
        _check(self.lib, self.lib.efa_comm_destroy(self.handle))

    def allreduce_sum(self, buf, count):
        """buf[count] (device, float64) <- sum over the ranks, in place, on the context's stream."""
        _check(self.lib, self.lib.efa_allreduce_sum_dev(self.handle, self._addr(buf), int(count)))

    def gc_block_counts(self, grid_lat, grid_lon, ob_lat, ob_lon, ob_halfwidth, ob_assim):
        """Per block of 16 (y,x) columns under Gaspari-Cohn localisation: the length of its active list and its
        (column, ob) pairs with a non-zero weight; and the total of the pairs."""
        glat = np.ascontiguousarray(grid_lat, dtype=np.float64).reshape(-1)
        glon = np.ascontiguousarray(grid_lon, dtype=np.float64).reshape(-1)
        ncol = glat.shape[0]
        P = len(ob_lat)
        lat = np.ascontiguousarray(ob_lat, dtype=np.float64).reshape(P)
        lon = np.ascontiguousarray(ob_lon, dtype=np.float64).reshape(P)
        hw = np.ascontiguousarray(ob_halfwidth, dtype=np.float64).reshape(P)
        asm = np.ascontiguousarray(np.asarray(ob_assim).astype(bool), dtype=np.uint8).reshape(P)
        cnt = np.zeros((ncol + 15) // 16, dtype=np.int32)
        bp = np.zeros_like(cnt)
        pairs = ctypes.c_uint64(0)
        i32p = ctypes.POINTER(ctypes.c_int32)
        _check(self.lib, self.lib.efa_gc_block_counts(self.handle, ncol, _dp(glat), _dp(glon), P, _dp(lat), _dp(lon), _dp(hw),
                                                      _u8p(asm), cnt.ctypes.data_as(i32p), bp.ctypes.data_as(i32p),
                                                      ctypes.byref(pairs)))
        return cnt, bp, int(pairs.value)

    def fill_synthetic(self, rows, row_offset, M, seed, sigma, X):
        _check(self.lib, self.lib.efa_fill_synthetic_dev(self.handle, rows, row_offset, M, int(seed),
                                                         float(sigma), self._addr(X)))


_contexts = {}


def get_context(device=0):
    """Process-wide cached context per device."""
    device = int(device)
    ctx = _contexts.get(device)
    if ctx is None or ctx.handle is None:
        ctx = Context(device)
        _contexts[device] = ctx
    return ctx
