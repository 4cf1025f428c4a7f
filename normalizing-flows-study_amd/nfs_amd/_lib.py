"""ctypes binding of libnfx.so (the C-ABI declared in include/nfx.h).

The product path fails loudly when the library is missing: every HIP entry point goes through
`checked()` / `lib()`, which raise NfxLibraryError instead of silently falling back to eager
PyTorch. `_SIGNATURES` is the one table of the ABI; `lib()` binds it as plain ctypes (return
codes), `checked()` as calls that take tensors and raise NfxError on a failing status.
"""
import ctypes
import os
import threading
import types

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NFX_LIB", os.path.join(_HERE, "libnfx.so"))

NFX_OK = 0
NFX_EINVAL = -1
NFX_EUNSUPPORTED = -2
NFX_ELAUNCH = -3
NFX_FORWARD = 1
NFX_INVERSE = -1
NFX_MAF_INVERSE = 0
NFX_IAF_FORWARD = 1
NFX_MAF_FORWARD = 2
NFX_IAF_INVERSE = 3
NFX_AFFINE_AUTO = 0
NFX_AFFINE_STREAMING = 1
NFX_AFFINE_SMALL = 2
NFX_MADE_SEQ_AUTO = 0
NFX_MADE_SEQ_SEGMENT = 1
NFX_MADE_SEQ_WAVE = 2
NFX_MADE_SEQ_PUSH = 3
NFX_RESIDUAL_RELU = 0
NFX_RESIDUAL_ELU = 1
NFX_RESIDUAL_LEAKY_RELU = 2
NFX_RESIDUAL_TANH = 3
NFX_NAF_RELU = 0
NFX_NAF_ELU = 1
NFX_NAF_LEAKY_RELU = 2
NFX_NAF_GELU = 3
NFX_NAF_LAYER_NORM = 1


def NFX_NAF_RESIDUAL(l):
    """The nfx_naf_flow flag of hidden layer l being a residual block."""
    return 2 << l


class NfxLibraryError(RuntimeError):
    pass


class NfxError(RuntimeError):
    pass


class NfxMlpRaw(ctypes.Structure):
    """Mirror of `NfxMlpRaw` in include/nfx.h (device pointers of one conditioner MLP)."""
    _fields_ = [
        ("w", ctypes.c_void_p * 4),
        ("b", ctypes.c_void_p * 4),
        ("mask", ctypes.c_void_p * 4),
        ("bn_w", ctypes.c_void_p * 3),
        ("bn_b", ctypes.c_void_p * 3),
        ("bn_rm", ctypes.c_void_p * 3),
        ("bn_rv", ctypes.c_void_p * 3),
        ("bn_eps", ctypes.c_float),
        ("n_layers", ctypes.c_int),
    ]


class NfxNafLayer(ctypes.Structure):
    """Mirror of `NfxNafLayer` in include/nfx.h (device pointers of one DeepMADE layer)."""
    _fields_ = [
        ("weight", ctypes.c_void_p),
        ("bias", ctypes.c_void_p),
        ("mask", ctypes.c_void_p),
        ("ln_weight", ctypes.c_void_p),
        ("ln_bias", ctypes.c_void_p),
        ("ln_eps", ctypes.c_float),
        ("residual", ctypes.c_int),
    ]


class NfxNafLayerGrad(ctypes.Structure):
    """Mirror of `NfxNafLayerGrad` in include/nfx.h (device pointers of one DeepMADE layer's gradients)."""
    _fields_ = [
        ("weight", ctypes.c_void_p),
        ("bias", ctypes.c_void_p),
        ("ln_weight", ctypes.c_void_p),
        ("ln_bias", ctypes.c_void_p),
    ]


_vp = ctypes.c_void_p
_i64 = ctypes.c_int64
_int = ctypes.c_int
_f = ctypes.c_float
_sz = ctypes.c_size_t

_SIGNATURES = {
    "nfx_abi_version": (_int, []),
    "nfx_last_error": (ctypes.c_char_p, []),
    "nfx_last_kernel": (ctypes.c_char_p, []),
    "nfx_debug_fill_lds": (ctypes.c_int, [ctypes.c_uint32, ctypes.c_void_p]),
    "nfx_affine_packed_floats": (_sz, [_int, _int]),
    "nfx_affine_pack": (_int, [ctypes.POINTER(NfxMlpRaw), ctypes.POINTER(NfxMlpRaw), _vp, _int, _int, _vp, _vp]),
    "nfx_affine_coupling": (_int, [_vp, _vp, _vp, _vp, _i64, _int, _int, _int, _int, _vp]),
    "nfx_affine_coupling_logprob": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _int, _vp]),
    "nfx_affine_kernel_policy": (_int, [_int]),
    "nfx_linear_forward": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _int, _vp]),
    "nfx_linear_backward_data": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _int, _vp]),
    "nfx_linear_workspace_bytes": (_sz, [_i64, _int, _int]),
    "nfx_linear_backward_weight": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _vp, _vp]),
    "nfx_made_elem_forward": (_int, [_vp, _vp, _vp, _vp, _i64, _int, _int, _int, _vp]),
    "nfx_made_elem_step": (_int, [_vp, _vp, _vp, _vp, _i64, _int, _int, _int, _vp]),
    "nfx_made_elem_finish": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _int, _vp]),
    "nfx_made_elem_backward": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _vp]),
    "nfx_made_elem_seq_backward": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _int, _vp]),
    "nfx_made_elem_seq_step_backward": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _int,
                                               _vp]),
    "nfx_made_elem_prefix": (_int, [_vp, _vp, _i64, _int, _int, _vp]),
    "nfx_affine_elem_forward": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _int, _vp]),
    "nfx_affine_elem_backward": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _vp]),
    "nfx_bn_prepare": (_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_double, ctypes.c_double, _int, _int, _vp, _vp, _vp,
                              _vp, _vp]),
    "nfx_bn_apply_relu": (_int, [_vp, _vp, _vp, _vp, _i64, _int, _vp]),
    "nfx_arqs_step": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _int, _int, _int, _f, _f, _f,
                             _vp]),
    "nfx_bn_workspace_bytes": (_sz, [_i64, _int]),
    "nfx_bn_backward_sums": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _int, _vp, _vp]),
    "nfx_bn_backward_apply": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _vp, _i64, _int, _vp]),
    "nfx_spline_elem_forward": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _f, _f, _f, _f, _int, _int, _vp]),
    "nfx_spline_elem_backward": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _f, _f, _f, _f, _int,
                                        _vp]),
    "nfx_spline_elem_forward_bounded": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _f, _f, _f, _f, _int,
                                               _int, _vp]),
    "nfx_spline_elem_backward_bounded": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _f, _f, _f,
                                                _f, _int, _vp]),
    "nfx_spline_rescale": (_int, [_vp, _vp, _vp, _i64, _int, _f, _vp]),
    "nfx_arqs_bounds": (_int, [_vp, _vp, _vp, _i64, _int, _int, _vp]),
    "nfx_affine_chain_supported": (_int, [_i64, _int, _int]),
    "nfx_affine_chain": (_int, [ctypes.POINTER(_vp), _int, _vp, _vp, _vp, _i64, _int, _int, _int, _int, _vp]),
    "nfx_affine_chain_logprob": (_int, [ctypes.POINTER(_vp), _int, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _int, _int,
                                        _int, _vp]),
    "nfx_affine_chain_sample": (_int, [ctypes.POINTER(_vp), _int, ctypes.c_uint64, _vp, _vp, _vp, _vp, _i64, _int, _int,
                                       _vp]),
    "nfx_arqs_packed_floats": (_sz, [_int, _int, _int]),
    "nfx_arqs_pack": (_int, [ctypes.POINTER(NfxMlpRaw), _int, _int, _int, _vp, _vp]),
    "nfx_arqs": (_int, [_vp, _vp, _vp, _vp, _i64, _int, _int, _int, _f, _f, _f, _int, ctypes.c_double,
                        ctypes.c_double, _int, _int, _vp]),
    "nfx_spline_packed_floats": (_sz, [_int, _int, _int]),
    "nfx_spline_pack": (_int, [ctypes.POINTER(NfxMlpRaw), _vp, _int, _int, _int, _vp, _vp]),
    "nfx_spline_coupling": (_int, [_vp, _vp, _vp, _vp, _i64, _int, _int, _int, _f, _f, _f, _f,
                                   _int, _f, _f, _int, _int, _vp]),
    "nfx_spline_coupling_logprob": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _int, _f, _f,
                                           _f, _f, _int, _f, _f, _int, _vp]),
    "nfx_spline_chain_supported": (_int, [_i64, _int, _int, _int]),
    "nfx_spline_chain": (_int, [ctypes.POINTER(_vp), _int, _vp, _vp, _vp, _i64, _int, _int, _int, _f, _f, _f, _f,
                                _int, _int, _vp]),
    "nfx_spline_chain_logprob": (_int, [ctypes.POINTER(_vp), _int, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _int, _int,
                                        _int, _f, _f, _f, _f, _int, _vp]),
    "nfx_spline_chain_sample": (_int, [ctypes.POINTER(_vp), _int, ctypes.c_uint64, _vp, _vp, _vp, _vp, _i64, _int, _int,
                                       _int, _f, _f, _f, _f, _vp]),
    "nfx_cnf_packed_floats": (_sz, [_int, _int]),
    "nfx_cnf_pack": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _vp, _vp]),
    "nfx_cnf_supported": (_int, [_i64, _int, _int]),
    "nfx_cnf_integrate": (_int, [_vp, _vp, _vp, _vp, _i64, _int, _int, _f, _f, _f, _int, _vp]),
    "nfx_cnf_backward_supported": (_int, [_i64, _int, _int]),
    "nfx_cnf_backward_packed_floats": (_sz, [_int, _int]),
    "nfx_cnf_trajectory_floats": (_sz, [_i64, _int, _f, _f, _f]),
    "nfx_cnf_backward_workspace_floats": (_sz, [_i64, _int, _int]),
    "nfx_cnf_backward_slots": (_sz, [_i64, _int, _int]),
    "nfx_cnf_backward_block_threads": (_sz, [_i64, _int, _int]),
    "nfx_cnf_pack_backward": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _vp, _vp]),
    "nfx_cnf_integrate_save": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _f, _f, _f, _int, _vp]),
    "nfx_cnf_backward": (_int, [_vp] * 16 + [_i64, _int, _int, _f, _f, _f, _vp]),
    "nfx_residual_packed_floats": (_sz, [_int, _int]),
    "nfx_residual_supported": (_int, [_i64, _int, _int, _int]),
    "nfx_residual_pack": (_int, [_vp, _vp, _vp, _vp, _f] * 3 + [_int, _int, _vp, _vp]),
    "nfx_residual_flow": (_int, [_vp, _vp, _vp, _vp, _i64, _int, _int, _int, _int, _int, _int, _f, _int, _vp]),
    "nfx_residual_backward_supported": (_int, [_i64, _int, _int, _int]),
    "nfx_residual_backward_packed_floats": (_sz, [_int, _int]),
    "nfx_residual_backward_workspace_floats": (_sz, [_i64, _int, _int]),
    "nfx_residual_backward_slots": (_sz, [_i64, _int, _int]),
    "nfx_residual_backward_block_threads": (_sz, [_i64, _int, _int]),
    "nfx_residual_pack_backward": (_int, [_vp, _vp, _vp, _vp, _f] * 3 + [_int, _int, _vp, _vp]),
    "nfx_residual_backward": (_int, [_vp] * 12 + [_i64, _int, _int, _int, _int, _int, _vp]),
    "nfx_naf_packed_floats": (_sz, [_int, _int, _vp]),
    "nfx_naf_supported": (_int, [_i64, _int, _int, _vp, _int, _int]),
    "nfx_naf_pack": (_int, [_vp, _int, _int, _vp, _vp, _vp]),
    "nfx_naf_flow": (_int, [_vp, _vp, _vp, _vp, _i64, _int, _int, _vp, _int, _int, _f, _f, _int, _int, _vp]),
    "nfx_naf_wide_packed_floats": (_sz, [_int, _int, _vp]),
    "nfx_naf_wide_supported": (_int, [_i64, _int, _int, _vp, _int, _int]),
    "nfx_naf_wide_pack": (_int, [_vp, _int, _int, _vp, _vp, _vp]),
    "nfx_naf_wide_flow": (_int, [_vp, _vp, _vp, _vp, _i64, _int, _int, _vp, _int, _int, _f, _f, _int, _int, _vp]),
    "nfx_naf_backward_supported": (_int, [_i64, _int, _int, _vp, _int, _int]),
    "nfx_naf_backward_packed_floats": (_sz, [_int, _int, _vp]),
    "nfx_naf_pack_backward": (_int, [_vp, _int, _int, _vp, _vp, _vp]),
    "nfx_naf_backward_slots": (_sz, [_i64, _int, _int, _vp]),
    "nfx_naf_backward_block_threads": (_sz, [_i64, _int, _int, _vp]),
    "nfx_naf_backward_workspace_floats": (_sz, [_i64, _int, _int, _vp]),
    "nfx_naf_backward": (_int, [_vp] * 8 + [_i64, _int, _int, _vp, _int, _int, _f, _f, _vp]),
    "nfx_lowrank_supported": (_int, [_i64, _int, _int]),
    "nfx_lowrank_record_floats": (_sz, [_int]),
    "nfx_lowrank_pack_planar": (_int, [_vp, _vp, _vp, _int, _int, _f, _vp, _vp]),
    "nfx_lowrank_pack_radial": (_int, [_vp, _vp, _vp, _int, _int, _f, _vp, _vp]),
    "nfx_lowrank_pack_sylvester": (_int, [_vp, _vp, _vp, _int, _int, _int, _int, _f, _vp, _vp]),
    "nfx_lowrank_stack": (_int, [_vp, _int, _vp, _vp, _vp, _i64, _int, _int, _int, _vp]),
    "nfx_lrbwd_supported": (_int, [_i64, _int, _int, _int]),
    "nfx_lrbwd_max_layers": (_sz, [_int]),
    "nfx_lrbwd_chunk_rows": (_sz, [_int]),
    "nfx_lrbwd_slots": (_sz, [_i64, _int, _int]),
    "nfx_lrbwd_workspace_floats": (_sz, [_i64, _int, _int]),
    "nfx_lrbwd_stack": (_int, [_vp, _int, _vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _vp]),
    "nfx_lrbwd_param_grads": (_int, [_vp, _i64, _int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _vp]),
    "nfx_rqs_unit": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _int, _f, _f, _f, _int, _vp]),
    "nfx_rqs_unit_backward": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _int, _f, _f, _f, _int,
                                     _vp]),
    "nfx_made_packed_floats": (_sz, [_int, _int]),
    "nfx_made_pack": (_int, [ctypes.POINTER(NfxMlpRaw), _int, _int, _vp, _vp]),
    "nfx_made_pack_parallel": (_int, [ctypes.POINTER(NfxMlpRaw), _int, _int, _vp, _vp]),
    "nfx_made_pack_sequential": (_int, [_int, _int, _vp, _vp]),
    "nfx_made_seq_policy": (_int, [_int]),
    "nfx_base_normal": (_int, [ctypes.c_uint64, _vp, _vp, _i64, _int, _vp]),
    "nfx_made_sample_supported": (_int, [_int, _int, _int]),
    "nfx_made_affine_sample": (_int, [_vp, ctypes.c_uint64, _vp, _vp, _vp, _vp, _i64, _int, _int, _vp]),
    "nfx_made_affine": (_int, [_vp, _vp, _vp, _vp, _i64, _int, _int, _int, _int, _vp]),
    "nfx_made_affine_logprob": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _int, _int, _vp]),
    "nfx_made_pack_backward": (_int, [ctypes.POINTER(NfxMlpRaw), _int, _int, _vp, _vp]),
    "nfx_made_backward_factor_floats": (_sz, [_i64, _int, _int]),
    "nfx_made_backward_max_batch": (_i64, [_int, _int]),
    "nfx_made_affine_backward": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _int, _vp]),
    "nfx_made_seq_backward": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _int, _vp]),
    "nfx_made_factor_pitch": (_i64, [_i64]),
    "nfx_made_param_floats": (_sz, [_int, _int]),
    "nfx_made_wgrad_workspace_bytes": (_sz, [_i64, _int, _int]),
    "nfx_made_backward_weights": (_int, [_vp, _i64, _int, _int, ctypes.POINTER(_vp), _vp, _vp, _vp]),
    "nfx_affine_train_pack_floats": (_sz, [_int, _int]),
    "nfx_affine_train_stats_doubles": (_sz, [_int]),
    "nfx_affine_train_grad_doubles": (_sz, [_int, _int]),
    "nfx_affine_train_param_floats": (_sz, [_int, _int]),
    "nfx_affine_train_workspace_bytes": (_sz, [_i64, _int, _int]),
    "nfx_affine_train_pack": (_int, [ctypes.POINTER(NfxMlpRaw), ctypes.POINTER(NfxMlpRaw), _vp, _vp, _vp, _int,
                                     _int, _vp, _vp, _vp]),
    "nfx_affine_train_stats": (_int, [_vp, _vp, _i64, _int, _int, _int, _vp, _vp, _vp]),
    "nfx_affine_train_update_running": (_int, [_vp, _vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _int,
                                               ctypes.c_double, _vp]),
    "nfx_affine_train_update_running_counted": (_int, [_vp, _vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                                       ctypes.POINTER(_vp), _int, ctypes.c_double, _vp]),
    "nfx_affine_train_backward": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _int, _int, _vp, _vp, _vp,
                                         _vp]),
    "nfx_affine_train_assemble": (_int, [_vp, _vp, _vp, _int, _int, _f, _vp, _vp]),
    "nfx_affine_train_keep_floats": (_sz, [_i64, _int, _int]),
    "nfx_affine_train_stats_keep": (_int, [_vp, _vp, _i64, _int, _int, _int, _vp, _vp, _vp, _vp]),
    "nfx_affine_train_backward_keep": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _int, _int, _vp, _vp,
                                              _vp, _vp, _vp]),
    "nfx_affine_train_output": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _int, _vp]),
    "nfx_affine_eval_stats": (_int, [ctypes.POINTER(_vp), ctypes.POINTER(_vp), _int, _vp, _vp, _vp]),
    "nfx_spline_backward_packed_floats": (_sz, [_int, _int, _int]),
    "nfx_spline_backward_param_floats": (_sz, [_int, _int, _int]),
    "nfx_spline_backward_workspace_bytes": (_sz, [_i64, _int, _int, _int]),
    "nfx_spline_pack_backward": (_int, [ctypes.POINTER(NfxMlpRaw), _vp, _int, _int, _int, _vp, _vp]),
    "nfx_spline_coupling_backward": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _int, _int, _int, _int,
                                            _f, _f, _f, _f, _int, _vp]),
    "nfx_gauss_workspace_bytes": (_sz, [_i64]),
    "nfx_gauss_workspace_init": (_int, [_vp, _vp]),
    "nfx_gauss_logprob": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _int, _vp]),
    "nfx_gauss_logprob_backward": (_int, [_vp, _vp, _vp, _vp, _i64, _int, _vp]),
    "nfx_flowbn_workspace_bytes": (_sz, [_i64, _int]),
    "nfx_flowbn_apply": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _i64, _int, _int, _vp]),
    "nfx_flowbn_moments": (_int, [_vp, _i64, _int, _vp, _vp, _vp]),
    "nfx_flowbn_update_running": (_int, [_vp, _vp, _vp, ctypes.c_double, _int, _vp]),
    "nfx_flowbn_backward": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _i64, _int, _int,
                                   _vp, _vp]),
}

# Every symbol include/nfx.h declares (tests check the table against the header, type by type,
# and that the built library exports all of them).
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

# The c_int symbols whose return is a value (a version, a policy, a yes/no), not an NFX_* status;
# every other c_int symbol returns a status, which the checked handle turns into NfxError.
_VALUE_RETURNING = frozenset((
    "nfx_abi_version", "nfx_affine_kernel_policy", "nfx_made_seq_policy", "nfx_affine_chain_supported",
    "nfx_spline_chain_supported", "nfx_cnf_supported", "nfx_cnf_backward_supported",
    "nfx_made_sample_supported", "nfx_residual_supported", "nfx_residual_backward_supported",
    "nfx_naf_supported", "nfx_naf_wide_supported", "nfx_naf_backward_supported",
    "nfx_lowrank_supported", "nfx_lrbwd_supported"))


_as_pointer = _vp.from_param  # (an int as a full-width pointer argument, without a c_void_p object)


class DevicePtr:
    """argtype of the checked handle for a `void*`: None (null), anything with .data_ptr() (a
    tensor), or a plain int (a stream handle, an address the caller already holds)."""

    @staticmethod
    def from_param(v):
        # (every launch passes its stream as an int: tested for, an exception would cost ~0.4 us)
        if v is None or type(v) is int:
            return _as_pointer(v)
        return _as_pointer(v.data_ptr())


def _raise_on_status(rc, fn, args):
    if rc != NFX_OK:
        raise NfxError(f"{fn.__name__} failed (rc={rc}): {lib().nfx_last_error().decode(errors='replace')}")
    return rc


_lock = threading.Lock()
_lib = None
_checked = None


def load(path=LIB_PATH):
    """Load libnfx.so without touching the GPU (safe on CPU-only hosts)."""
    global _lib, _checked
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(path):
            raise NfxLibraryError(
                f"libnfx.so not found at {path}: build it with "
                f"`python normalizing-flows-study_amd/build.py` (or __graft_entry__.build()). "
                f"The HIP path has no eager fallback.")
        l = ctypes.CDLL(path)
        n = types.SimpleNamespace()
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(l, name, None)
            if fn is None:
                continue
            fn.restype = res
            fn.argtypes = args
            # a second pointer to the same symbol (getattr would return the raw one again)
            cf = l._FuncPtr((name, l))
            cf.__name__ = name
            cf.restype = res
            cf.argtypes = [DevicePtr if a is _vp else a for a in args]
            if res is _int and name not in _VALUE_RETURNING:
                cf.errcheck = _raise_on_status
            setattr(n, name, cf)
        _checked = n
        _lib = l
        return l


def lib():
    """The raw handle: plain ctypes functions, integer return codes, c_void_p arguments."""
    l = _lib
    return l if l is not None else load()


def checked():
    """The checked handle the product path launches through: the same symbols, but pointer
    arguments take tensors (DevicePtr) and a status other than NFX_OK raises NfxError."""
    if _checked is None:
        load()
    return _checked


def available():
    try:
        load()
        return True
    except NfxLibraryError:
        return False


def check(rc, what):
    if rc != NFX_OK:
        msg = lib().nfx_last_error().decode(errors="replace")
        raise NfxError(f"{what} failed (rc={rc}): {msg}")


def dense(t):
    """`t` in the form the kernels read a caller's tensor in: contiguous row-major, based at a
    16-byte boundary (x rows of d = 2 / 4 and packed images move as 8- and 16-byte loads). What
    the allocator hands out already is, and comes back as it is; a strided or transposed view is
    copied, and so is a contiguous view that starts at an odd float of a larger buffer.
    `DevicePtr` reads nothing but `data_ptr()`, so every tensor a caller owns passes through here
    (or `.contiguous()`, for the entry points that take any 4-byte-aligned base) on its way in."""
    t = t.contiguous()
    if t.data_ptr() & 15:
        t = t.clone()
    return t


def ptr(t):
    """Device address of a tensor as a plain int (ctypes c_void_p arguments accept ints)."""
    return None if t is None else t.data_ptr()


try:
    _raw_stream = torch._C._cuda_getCurrentRawStream
except AttributeError:  # pragma: no cover - older torch
    _raw_stream = None


def stream_of(t):
    """hipStream_t of torch's current stream on t's device (the stream kernels are enqueued on)."""
    if _raw_stream is not None and t.device.type == "cuda":
        return _raw_stream(t.device.index if t.device.index is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(t.device).cuda_stream


def mlp_raw(linears, batchnorms=(), masks=None):
    """Build an NfxMlpRaw from nn.Linear modules (+ optional BatchNorm1d after hidden layers).

    Returns (struct, keepalive) — keepalive holds the contiguous tensors the pointers refer to.
    """
    raw = NfxMlpRaw()
    keep = []

    def p(t):
        t = dense(t.detach().float())
        keep.append(t)
        return t.data_ptr()

    raw.n_layers = len(linears)
    for i, lin in enumerate(linears):
        raw.w[i] = p(lin.weight)
        raw.b[i] = p(lin.bias) if lin.bias is not None else None
        if masks is not None and masks[i] is not None:
            raw.mask[i] = p(masks[i])
    eps = 1e-5
    for i, bn in enumerate(batchnorms):
        if bn is None:
            continue
        raw.bn_w[i] = p(bn.weight) if bn.weight is not None else p(torch.ones_like(bn.running_var))
        raw.bn_b[i] = p(bn.bias) if bn.bias is not None else p(torch.zeros_like(bn.running_var))
        raw.bn_rm[i] = p(bn.running_mean)
        raw.bn_rv[i] = p(bn.running_var)
        eps = bn.eps
    raw.bn_eps = eps
    return raw, keep


def last_kernel():
    """Name of the last kernel this thread launched through libnfx (profiling aid)."""
    return lib().nfx_last_kernel().decode()
