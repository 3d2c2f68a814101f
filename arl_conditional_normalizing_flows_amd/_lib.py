"""ctypes binding of libcnf_hip.so (include/cnf.h).

This is the reference-side binding a Python caller uses: every entry point of the C ABI is
declared here with its argument types. The library is REQUIRED: there is no CPU fallback on
the product path; a missing or unloadable library raises immediately.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

_PKG = Path(__file__).resolve().parent
# CNF_LIB: load an alternative build of the same library (kernel-variant experiments)
LIB_PATH = Path(os.environ['CNF_LIB']) if os.environ.get('CNF_LIB') else _PKG / 'lib' / 'libcnf_hip.so'


class cnf_flow_desc(C.Structure):
    _fields_ = [('io_h', C.c_int), ('io_w', C.c_int), ('io_d', C.c_int), ('x_d', C.c_int),
                ('num_blocks', C.c_int),
                ('squeeze_factor_block_list', C.POINTER(C.c_int)),
                ('resnext_block_list', C.POINTER(C.c_int)),
                ('num_kernels_list', C.POINTER(C.c_int)),
                ('cardinality_list', C.POINTER(C.c_int)),
                ('lambda_y', C.c_float), ('ksize', C.c_int), ('layer_norm', C.c_int),
                ('dilations', C.c_int), ('group_mode', C.c_int), ('debug_options', C.c_char_p)]


class cnf_layer_info(C.Structure):
    _fields_ = [('kind', C.c_int), ('coupling_index', C.c_int), ('block', C.c_int),
                ('h', C.c_int), ('w', C.c_int), ('d', C.c_int), ('mask', C.c_int),
                ('hc', C.c_int), ('wc', C.c_int), ('dc1', C.c_int), ('dc2', C.c_int),
                ('num_kernels', C.c_int), ('cardinality', C.c_int), ('num_res_blocks', C.c_int),
                ('num_dilations', C.c_int), ('dilations', C.c_int * 8), ('num_prev_factors', C.c_int),
                ('fused_net', C.c_int)]


class cnf_toy_desc(C.Structure):
    _fields_ = [('io_shape', C.c_int), ('x_d', C.c_int), ('num_coupling_layers', C.c_int),
                ('intermediate_dims', C.c_int), ('num_layers', C.c_int), ('mask_indices', C.POINTER(C.c_int)),
                ('lambda_y', C.c_float)]


class cnf_sample_desc(C.Structure):
    _fields_ = [('num_samples', C.c_int), ('chunk', C.c_int), ('temperature', C.c_float),
                ('seed', C.c_uint64), ('offset', C.c_uint64), ('logit_a', C.c_float), ('residual', C.c_int)]


class cnf_sample_score_desc(C.Structure):
    _fields_ = [('bins', C.c_int), ('lo', C.c_float), ('hi', C.c_float), ('num_quantiles', C.c_int),
                ('quantiles', C.c_float * 8)]


class cnf_cascade_desc(C.Structure):
    _fields_ = [('num_stages', C.c_int), ('num_samples', C.c_int * 4), ('chunk', C.c_int),
                ('temperature', C.c_float * 4), ('seed', C.c_uint64), ('offset', C.c_uint64 * 4),
                ('logit_a', C.c_float), ('residual', C.c_int)]


class cnf_logp_desc(C.Structure):
    _fields_ = [('num_conditions', C.c_int), ('chunk', C.c_int), ('logit_a', C.c_float), ('residual', C.c_int)]


class cnf_score_desc(C.Structure):
    _fields_ = [('chunk', C.c_int), ('logit_a', C.c_float), ('residual', C.c_int)]


class cnf_ascend_desc(C.Structure):
    _fields_ = [('chunk', C.c_int), ('steps', C.c_int), ('lr', C.c_float), ('beta_1', C.c_float),
                ('beta_2', C.c_float), ('epsilon', C.c_float), ('logit_a', C.c_float), ('residual', C.c_int),
                ('first_step', C.c_int)]


class cnf_optim_desc(C.Structure):
    _fields_ = [('lr', C.c_float), ('beta_1', C.c_float), ('beta_2', C.c_float), ('epsilon', C.c_float),
                ('clipvalue', C.c_float), ('clipnorm', C.c_float), ('global_clipnorm', C.c_float),
                ('skip_nonfinite', C.c_int), ('ema_momentum', C.c_float)]


OPTIM_STATS_FLOATS = 8   # CNF_OPTIM_STATS_FLOATS


class cnf_batch_desc(C.Structure):
    _fields_ = [('H', C.c_int), ('W', C.c_int), ('C', C.c_int), ('mode', C.c_int), ('logit_a', C.c_float),
                ('x_down', C.c_int), ('y_levels', C.c_int), ('residual', C.c_int),
                ('alpha0', C.c_float), ('seed0', C.c_uint64), ('offset0', C.c_uint64),
                ('alpha1', C.c_float), ('seed1', C.c_uint64), ('offset1', C.c_uint64)]


BATCH_CLASS, BATCH_SR = 0, 1   # CNF_BATCH_CLASS, CNF_BATCH_SR


class cnf_toy_sample_desc(C.Structure):
    _fields_ = [('num_samples', C.c_int), ('temperature', C.c_float), ('seed', C.c_uint64), ('offset', C.c_uint64),
                ('hist_bins', C.c_int), ('hist_lo', C.c_float * 2), ('hist_hi', C.c_float * 2)]


class cnf_toy_density_desc(C.Structure):
    _fields_ = [('num_points', C.c_int), ('grid_bins', C.c_int), ('lo', C.c_float * 2), ('hi', C.c_float * 2)]


# per-layer completion callback of cnf_flow_backward_ex (void (*)(void* user, int coupling_index))
LAYER_DONE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int)

# (name, restype, argtypes)
_P = C.c_void_p
_F = C.c_void_p   # device float* as integer address
_SIGS = [
    ('cnf_plan_create', C.c_int, [C.POINTER(cnf_flow_desc), C.POINTER(_P)]),
    ('cnf_plan_destroy', None, [_P]),
    ('cnf_plan_num_layers', C.c_int, [_P]),
    ('cnf_plan_layer_info', C.c_int, [_P, C.c_int, C.POINTER(cnf_layer_info)]),
    ('cnf_plan_num_params', C.c_int64, [_P]),
    ('cnf_plan_num_param_tensors', C.c_int, [_P]),
    ('cnf_plan_param_tensor', C.c_int, [_P, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int64),
                                        C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ('cnf_plan_aux_floats', C.c_int64, [_P]),
    ('cnf_pack_params', C.c_int, [_P, _F, _F, _P]),
    ('cnf_plan_workspace_bytes', C.c_size_t, [_P, C.c_int]),
    ('cnf_flow_forward', C.c_int, [_P, _F, _F, _F, _F, _F, _P, C.c_int, _P]),
    ('cnf_flow_forward_noise', C.c_int, [_P, _F, _F, _F, C.c_float, C.c_float, C.c_uint64, C.c_uint64, _F, _F, _F, _P,
                                         C.c_int, _P]),
    ('cnf_flow_inverse', C.c_int, [_P, _F, _F, _F, _F, _P, C.c_int, _P]),
    ('cnf_flow_inverse_logdet', C.c_int, [_P, _F, _F, _F, _F, _F, _P, C.c_int, _P]),
    ('cnf_plan_sample_workspace_bytes', C.c_size_t, [_P, C.c_int, C.POINTER(cnf_sample_desc)]),
    ('cnf_flow_sample', C.c_int, [_P, _F, _F, _F, C.POINTER(cnf_sample_desc), _F, _F, _F, _F, _P, C.c_int, _P]),
    ('cnf_flow_sample_logp', C.c_int, [_P, _F, _F, _F, C.POINTER(cnf_sample_desc), _F, _F, _F, _F, _F, _P, C.c_int,
                                       _P]),
    ('cnf_flow_sample_score', C.c_int, [_P, _F, _F, _F, C.POINTER(cnf_sample_desc), C.POINTER(cnf_sample_score_desc),
                                        _F, _F, _F, _F, _F, _F, _F, _F, _F, _F, _F, _P, C.c_int, _P]),
    ('cnf_cascade_workspace_bytes', C.c_size_t, [C.POINTER(_P), C.c_int, C.POINTER(cnf_cascade_desc)]),
    ('cnf_flow_sample_cascade', C.c_int, [C.POINTER(_P), C.POINTER(_F), C.POINTER(_F), _F, C.POINTER(cnf_cascade_desc),
                                          C.POINTER(cnf_sample_score_desc), _F, _F, _F, _F, _F, _F, _F, C.POINTER(_F),
                                          C.POINTER(_F), C.POINTER(_F), C.POINTER(_F), _P, C.c_int, _P]),
    ('cnf_plan_logp_workspace_bytes', C.c_size_t, [_P, C.c_int, C.POINTER(cnf_logp_desc)]),
    ('cnf_flow_log_prob', C.c_int, [_P, _F, _F, _F, _F, C.POINTER(cnf_logp_desc), _F, _F, _F, _F, _F, _F, _F, _F, _P,
                                    C.c_int, _P]),
    ('cnf_plan_score_workspace_bytes', C.c_size_t, [_P, C.c_int, C.POINTER(cnf_score_desc)]),
    ('cnf_flow_score', C.c_int, [_P, _F, _F, _F, _F, C.POINTER(cnf_score_desc), _F, _F, _F, _P, C.c_int, _P]),
    ('cnf_plan_ascend_workspace_bytes', C.c_size_t, [_P, C.c_int, C.POINTER(cnf_ascend_desc)]),
    ('cnf_flow_ascend', C.c_int, [_P, _F, _F, _F, _F, C.POINTER(cnf_ascend_desc), _F, _F, _F, _F, _P, C.c_int, _P]),
    ('cnf_coupling_forward', C.c_int, [_P, C.c_int, _F, _F, _F, _F, _F, _P, C.c_int, _P]),
    ('cnf_coupling_inverse', C.c_int, [_P, C.c_int, _F, _F, _F, _F, _P, C.c_int, _P]),
    ('cnf_coupling_inverse_logdet', C.c_int, [_P, C.c_int, _F, _F, _F, _F, _F, _P, C.c_int, _P]),
    ('cnf_squeeze', C.c_int, [_F, _F, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    ('cnf_channel_copy', C.c_int, [_F, C.c_int, C.c_int, _F, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_int, _P]),
    ('cnf_nll', C.c_int, [_P, _F, _F, _F, _F, _F, C.c_int, _P]),
    ('cnf_plan_train_workspace_bytes', C.c_size_t, [_P, C.c_int]),
    ('cnf_flow_forward_train', C.c_int, [_P, _F, _F, _F, _F, _F, _P, C.c_int, _P]),
    ('cnf_flow_backward', C.c_int, [_P, _F, _F, _F, _P, C.c_int, C.c_float, _F, _P]),
    ('cnf_flow_backward_ex', C.c_int, [_P, _F, _F, _F, _P, C.c_int, _F, _F, LAYER_DONE_FN, _P, _P]),
    ('cnf_coupling_backward', C.c_int, [_P, C.c_int, _F, _F, _F, _F, C.c_float, _P, C.c_int, _F, _P]),
    ('cnf_adam_step', C.c_int, [_F, _F, _F, _F, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int,
                                _P]),
    ('cnf_optim_slab_elems', C.c_int, []),
    ('cnf_optim_num_slabs', C.c_int64, [C.c_int64, C.POINTER(C.c_int64), C.c_int]),
    ('cnf_optim_table_bytes', C.c_size_t, [C.c_int64, C.POINTER(C.c_int64), C.c_int]),
    ('cnf_optim_table_build', C.c_int, [C.c_int64, C.POINTER(C.c_int64), C.c_int, _P]),
    ('cnf_optim_workspace_bytes', C.c_size_t, [C.c_int64, C.c_int, C.c_int64]),
    ('cnf_optim_step', C.c_int, [_F, _F, _F, _F, _F, C.c_int64, _P, C.c_int64, C.c_int, C.POINTER(cnf_optim_desc),
                                 _P, _F, _F, _P, _P]),
    ('cnf_toy_num_params', C.c_int64, [C.POINTER(cnf_toy_desc)]),
    ('cnf_toy_call', C.c_int, [C.POINTER(cnf_toy_desc), _F, _F, _F, _F, _F, C.c_int, C.c_int, _P]),
    ('cnf_toy_nll_sums', C.c_int, [_F, _F, C.c_int, _P]),
    ('cnf_toy_train_workspace_bytes', C.c_size_t, [C.POINTER(cnf_toy_desc), C.c_int]),
    ('cnf_toy_forward_train', C.c_int, [C.POINTER(cnf_toy_desc), _F, _F, _F, _F, _P, C.c_int, _P]),
    ('cnf_toy_backward', C.c_int, [C.POINTER(cnf_toy_desc), _F, _F, _F, _P, C.c_int, C.c_float, _F, _P]),
    ('cnf_toy_sample_workspace_bytes', C.c_size_t, [C.POINTER(cnf_toy_desc), C.c_int, C.POINTER(cnf_toy_sample_desc)]),
    ('cnf_toy_sample', C.c_int, [C.POINTER(cnf_toy_desc), _F, _F, C.POINTER(cnf_toy_sample_desc), _F, _F, _F, _F, _F, _P,
                                 C.c_int, _P]),
    ('cnf_toy_density_workspace_bytes', C.c_size_t, [C.POINTER(cnf_toy_desc), C.c_int,
                                                     C.POINTER(cnf_toy_density_desc)]),
    ('cnf_toy_density', C.c_int, [C.POINTER(cnf_toy_desc), _F, _F, _F, C.POINTER(cnf_toy_density_desc), _F, _F, _F, _F,
                                  _P, C.c_int, _P]),
    ('cnf_logit', C.c_int, [_F, _F, C.c_int64, C.c_float, C.c_int, _P]),
    ('cnf_sr_preprocess', C.c_int, [_F, _F, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    ('cnf_down', C.c_int, [_F, _F, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    ('cnf_up', C.c_int, [_F, _F, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    ('cnf_instance_noise', C.c_int, [_F, _F, C.c_int64, C.c_float, C.c_uint64, C.c_uint64, _P]),
    ('cnf_batch_assemble', C.c_int, [_F, C.c_int64, _P, _F, C.POINTER(cnf_batch_desc), _F, C.c_int, _P]),
    ('cnf_plan_num_recorded_launches', C.c_int, [_P]),
    ('cnf_plan_recorded_launch_info', C.c_int, [_P, C.c_int, C.c_char_p, C.c_int,
                                                C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ('cnf_plan_relaunch', C.c_int, [_P, C.c_int, _P]),
    ('cnf_plan_set_launch_timing', C.c_int, [_P, C.c_int]),
    ('cnf_plan_launch_time_ms', C.c_int, [_P, C.c_int, C.POINTER(C.c_float)]),
    ('cnf_plan_weight_map', C.c_int64, [_P, C.c_int, C.POINTER(C.c_int64), C.c_int64]),
    ('cnf_comm_unique_id', C.c_int, [C.c_char_p]),
    ('cnf_comm_init', C.c_int, [C.c_int, C.c_int, C.c_char_p, C.POINTER(_P)]),
    ('cnf_comm_destroy', None, [_P]),
    ('cnf_allreduce_sum_f32', C.c_int, [_P, _F, C.c_size_t, _P]),
    ('cnf_nll_allreduce', C.c_int, [_P, _F, C.c_int, _F, _P]),
    ('cnf_last_error', C.c_char_p, []),
    ('cnf_version', C.c_char_p, []),
]

EXPORTED_SYMBOLS = [s[0] for s in _SIGS]

# introspection entry points outside include/cnf.h (csrc/cnf_debug.cpp): host only, nothing is launched
_I = C.POINTER(C.c_int)
_DEBUG_SIGS = [
    # the training backward's batch partitions, from the host functions the launch code calls
    ('cnf_debug_train_convs', C.c_int, [_P, C.c_int, _I, C.c_int]),
    ('cnf_debug_wgrad_choice', C.c_int, [_P] + [C.c_int] * 8 + [_I, C.c_int]),
    ('cnf_debug_tconv_choice', C.c_int, [_P] + [C.c_int] * 11 + [_I, C.c_int]),
    ('cnf_debug_lnb_slicing', C.c_int, [C.c_longlong, C.c_int, _I, C.c_int]),
    ('cnf_debug_grad_rows_trips', C.c_int, [C.c_int]),
    # the forward's k_pw launch shapes (a host-only dry run) and the images a workgroup of one loops over
    ('cnf_debug_pw_shapes', C.c_int, [_P, C.c_int, _I, C.c_int]),
    ('cnf_debug_pw_words', C.c_int, []),
    ('cnf_debug_pw_ipw', C.c_int, [C.c_int] * 4),
    # what cnf_flow_log_prob launches for a chunk of n pairs (gather kernel, tiles, grid, finish trips)
    ('cnf_debug_logp_choice', C.c_int, [_P, C.c_int, C.c_int, _I, C.c_int]),
]

_lib = None


class CnfError(RuntimeError):
    pass


def load(path: os.PathLike | str | None = None):
    """Load libcnf_hip.so (raises if absent: the HIP path is mandatory)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = Path(path) if path is not None else LIB_PATH
    if not p.exists():
        raise CnfError(f'{p} is missing: build it with `python -m arl_conditional_normalizing_flows_amd._build` '
                       f'(hipcc --offload-arch=gfx950). There is no CPU fallback.')
    # torch's wheel carries its own HIP / HSA runtime. Loaded after this library, it is a second
    # runtime in the process next to the system one this library resolved, and the library's calls
    # then find no device; loaded first, its libamdhip64 satisfies this library's dependency too.
    try:
        import torch  # noqa: F401
    except ImportError:   # a caller without torch: the system runtime is the only one
        pass
    lib = C.CDLL(str(p))
    for name, res, args in _SIGS + _DEBUG_SIGS:
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def check(rc: int, what: str = ''):
    if rc != 0:
        if rc == -1:
            raise AssertionError(f'{what}: {load().cnf_last_error().decode()}')
        raise CnfError(f'{what} failed ({rc}): {load().cnf_last_error().decode()}')


def ptr(t) -> int:
    """device pointer of a contiguous torch tensor (or None -> NULL)."""
    if t is None:
        return None
    return t.data_ptr()
