"""Drop-in replacement for the reference's `conv_cINN_make_model` layer/model API on MI355X.

Same class names, constructor arguments, method names, argument order, return values and
`None` conventions as conv_cINN_make_model.py; tensors are torch tensors on the ROCm device
(NHWC, contiguous, float32) instead of TF tensors. Every computation runs in
libcnf_hip.so (hand-written gfx950 HIP kernels) through the C ABI in include/cnf.h — there is
no CPU or torch-op fallback: if the library is missing the constructor raises.

Reference map
  Layer                    conv_cINN_make_model.py:62-89
  tanh_scaling_layer       :97-122  (a scalar parameter inside net A; exposed for API parity)
  squeeze_layer            :130-217
  factor_out_zy_layer      :219-329
  coupling_layer           :337-1394
  cFlow                    :1408-1904
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr

GROUP_MODES = {'reference': 0, 'intended': 1}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _as_input(t, what='input'):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f'{what} must be a torch.Tensor on the ROCm device')
    if not t.is_cuda:
        raise ValueError(f'{what} must live on the GPU (got {t.device}); the HIP path has no CPU fallback')
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _call_workspace(cache, key, device, who, nbytes):
    """cache[key], or a new workspace of nbytes() bytes; <= 0: an argument error, as the reference's asserts"""
    ws = cache.get(key)
    if ws is None:
        n = int(nbytes())
        if n <= 0:
            raise AssertionError(f'{who}: {_lib.load().cnf_last_error().decode()}')
        ws = cache[key] = torch.empty(n, device=device, dtype=torch.uint8)
    return ws


def _score_setup(out, shape, S, device, truth, hist, quantiles, return_sq_err):
    """The score arguments of sample(): checks truth [B,H,W,x_d] = shape, allocates the requested score outputs
    into `out` for S draws per condition, and returns (cnf_sample_score_desc, truth)."""
    B, H, W, x_d = shape
    sd = _lib.cnf_sample_score_desc()
    if truth is not None:
        truth = _as_input(truth, 'truth')
        if truth.dim() == 3:
            truth = truth.unsqueeze(0)
        if tuple(truth.shape) != (B, H, W, x_d):
            raise ValueError(f'truth has shape {tuple(truth.shape)}, expected [{B}, {H}, {W}, {x_d}]')
        out['rank'] = torch.empty((B, H, W, x_d), device=device, dtype=torch.int32)
        out['abs_err'] = torch.empty((B, H, W, x_d), device=device, dtype=torch.float32)
        if return_sq_err is None or return_sq_err:
            out['sq_err'] = torch.empty((B, max(S, 0)), device=device, dtype=torch.float32)
    elif return_sq_err:
        raise AssertionError('cFlow.sample: return_sq_err needs truth')
    if hist is not None:
        bins, lo, hi = hist
        sd.bins, sd.lo, sd.hi = int(bins), float(lo), float(hi)
        if not 2 <= sd.bins <= 256:   # (before the allocation below is sized by it)
            raise AssertionError(f'cFlow.sample: hist bins must be in 2..256, got {bins}')
        out['hist'] = torch.empty((B, H, W, x_d, sd.bins), device=device, dtype=torch.int32)
        k = torch.arange(sd.bins, device=device, dtype=torch.float32)
        out['hist_centers'] = sd.lo + (k + 0.5) * ((sd.hi - sd.lo) / sd.bins)
    if quantiles is not None:
        if hist is None:
            raise AssertionError('cFlow.sample: quantiles needs hist=(bins, lo, hi)')
        levels = [float(q) for q in quantiles]
        if not 1 <= len(levels) <= 8:
            raise AssertionError(f'cFlow.sample: 1..8 quantile levels, got {len(levels)}')
        sd.num_quantiles = len(levels)
        for j, q in enumerate(levels):
            sd.quantiles[j] = q
        out['quantiles'] = torch.empty((len(levels), B, H, W, x_d), device=device, dtype=torch.float32)
    return sd, truth


# ---------------------------------------------------------------------------------------------
# layers
# ---------------------------------------------------------------------------------------------

class Layer:
    """Abstract two-direction layer (conv_cINN_make_model.py:62-89)."""

    def forward_and_Jacobian(self, u, sum_log_det_J, z):
        raise NotImplementedError(str(type(self)))

    def backward(self, v, z):
        raise NotImplementedError(str(type(self)))


def _accumulate_logdet(sum_log_det_J, per_image):
    """Reference semantics: sum_log_detJ += reduce_mean(reduce_sum(A(u1))) (:1323-1326).
    If the caller passes a per-image (B,) tensor, accumulate per image instead."""
    if isinstance(sum_log_det_J, torch.Tensor) and sum_log_det_J.dim() == 1 \
            and sum_log_det_J.shape[0] == per_image.shape[0]:
        return sum_log_det_J + per_image
    return sum_log_det_J + per_image.mean()


class tanh_scaling_layer(Layer):
    """Scalar multiplier after tanh in net A (:97-122). In this implementation the scalar is
    parameter `c{i}.A.tanh_scale.w` of the owning cFlow and is applied inside k_coupling."""

    def __init__(self, flow=None, coupling_index=None):
        self._flow = flow
        self._ci = coupling_index

    @property
    def w(self):
        return self._flow.get_param(f'c{self._ci}.A.tanh_scale.w')

    def call(self, inputs):
        return self.w * inputs


class squeeze_layer(Layer):
    """space_to_depth(2) / depth_to_space(2) on u and zy (:130-217), TF channel order."""

    def forward_and_Jacobian(self, u, sum_log_det_J, zy):
        u = _as_input(u, 'u')
        assert u.shape[1] % 2 == 0 and u.shape[2] % 2 == 0, 'u must have spatial dimensions divisible by 2.'
        v = _squeeze(u, +1)
        if zy is not None:
            zy = _squeeze(_as_input(zy, 'zy'), +1)
        return v, sum_log_det_J, zy

    def backward(self, v, zy):
        v = _as_input(v, 'v')
        assert v.shape[3] % 4 == 0, 'v must have channel dimensions divisible by 4.'
        u = _squeeze(v, -1)
        if zy is not None:
            zy = _squeeze(_as_input(zy, 'zy'), -1)
        return u, zy


def _squeeze(x, direction):
    B, H, W, Cc = x.shape
    if direction > 0:
        out = torch.empty((B, H // 2, W // 2, 4 * Cc), device=x.device, dtype=torch.float32)
    else:
        out = torch.empty((B, 2 * H, 2 * W, Cc // 4), device=x.device, dtype=torch.float32)
    if x.numel() > 0:
        check(_lib.load().cnf_squeeze(ptr(x), ptr(out), B, H, W, Cc, direction, _stream()), 'cnf_squeeze')
    return out


def _channels(x, start, stop):
    """x[..., start:stop] as a new contiguous tensor (HIP channel copy)."""
    B, H, W, Cc = x.shape
    n = stop - start
    out = torch.empty((B, H, W, n), device=x.device, dtype=torch.float32)
    if n > 0 and B * H * W > 0:
        check(_lib.load().cnf_channel_copy(ptr(x), Cc, start, ptr(out), n, 0, n, B, H * W, _stream()),
              'cnf_channel_copy')
    return out


def _concat(a, b):
    """concat([a, b], axis=3) (HIP channel copies)."""
    B, H, W, ca = a.shape
    cb = b.shape[3]
    out = torch.empty((B, H, W, ca + cb), device=a.device, dtype=torch.float32)
    lib = _lib.load()
    if ca:
        check(lib.cnf_channel_copy(ptr(a), ca, 0, ptr(out), ca + cb, 0, ca, B, H * W, _stream()), 'concat')
    if cb:
        check(lib.cnf_channel_copy(ptr(b), cb, 0, ptr(out), ca + cb, ca, cb, B, H * W, _stream()), 'concat')
    return out


class factor_out_zy_layer(Layer):
    """Factor half of the channels out into zy / back in (:219-329)."""

    def __init__(self, num_prev_factors, **kwargs):
        self.num_prev_factors = int(num_prev_factors)

    def get_config(self):
        return {'num_prev_factors': self.num_prev_factors}

    def forward_and_Jacobian(self, u, sum_log_det_J, zy):
        u = _as_input(u, 'u')
        split = u.shape[3] // 2
        factored = _channels(u, 0, split)
        v = _channels(u, split, u.shape[3])
        zy = _concat(_as_input(zy, 'zy'), factored) if zy is not None else factored
        return v, sum_log_det_J, zy

    def backward(self, v, zy):
        zy = _as_input(zy, 'zy')
        if v is None:
            split = zy.shape[3] // (2 ** self.num_prev_factors)
        else:
            v = _as_input(v, 'v')
            split = v.shape[3]
        cz = zy.shape[3]
        re = _channels(zy, cz - split, cz)
        zy = _channels(zy, 0, cz - split)
        assert re.shape[3] == split
        u = _concat(re, v) if v is not None else re
        return u, zy


class coupling_layer(Layer):
    """Affine coupling layer with compressed checkerboard / channel masks and ResNeXt s,t
    networks (:337-1394). Instances are created by cFlow (they execute through the flow's
    plan and parameter buffers)."""

    def __init__(self, flow: 'cFlow', layer_index: int, info):
        self._flow = flow
        self._layer = layer_index
        self.coupling_index = info.coupling_index
        self.input_height, self.input_width, self.input_depth = info.h, info.w, info.d
        self.which_mask = info.mask
        self.which_mask_complement = {0: 1, 1: 0, 2: 3, 3: 2}[info.mask]
        self.num_res_blocks = info.num_res_blocks
        self.cardinality = info.cardinality
        self.num_kernels = info.num_kernels
        self.kernel_size = flow.ksize
        self.LAYER_NORM = flow.LAYER_NORM
        self.which_dilations = [info.dilations[i] for i in range(info.num_dilations)]
        self.compressed_height, self.compressed_width, self.compressed_depth = info.hc, info.wc, info.dc1
        self.uv2_depth = info.dc2
        self.tanh_scale = tanh_scaling_layer(flow, info.coupling_index)

    def get_config(self):
        return {'input_height': self.input_height, 'input_width': self.input_width,
                'input_depth': self.input_depth, 'which_mask': self.which_mask,
                'num_res_blocks': self.num_res_blocks, 'cardinality': self.cardinality,
                'kernel_size': self.kernel_size, 'LAYER_NORM': self.LAYER_NORM,
                'which_dilations': self.which_dilations}

    def _check(self, t, what):
        t = _as_input(t, what)
        # tf.ensure_shape(u, [None, H, W, D]) (:1276-1280, :1348-1352)
        if tuple(t.shape[1:]) != (self.input_height, self.input_width, self.input_depth):
            raise ValueError(f'{what} has shape {tuple(t.shape)}, expected [None, {self.input_height}, '
                             f'{self.input_width}, {self.input_depth}]')
        return t

    def forward_and_Jacobian(self, u, sum_log_detJ, zy):
        u = self._check(u, 'u')
        f = self._flow
        B = u.shape[0]
        v = torch.empty_like(u)
        ld = torch.zeros(B, device=u.device, dtype=torch.float32)
        ws = f._workspace(B)
        check(_lib.load().cnf_coupling_forward(f._plan, self._layer, ptr(f.params), ptr(f._aux), ptr(u), ptr(v),
                                               ptr(ld), ptr(ws), B, _stream()), 'cnf_coupling_forward')
        return v, _accumulate_logdet(sum_log_detJ, ld), zy

    def backward(self, v, zy):
        v = self._check(v, 'v')
        f = self._flow
        B = v.shape[0]
        u = torch.empty_like(v)
        ws = f._workspace(B)
        check(_lib.load().cnf_coupling_inverse(f._plan, self._layer, ptr(f.params), ptr(f._aux), ptr(v), ptr(u),
                                               ptr(ws), B, _stream()), 'cnf_coupling_inverse')
        return u, zy

    def backward_and_Jacobian(self, v, sum_log_det_J, zy):
        """backward that also accumulates this layer's log|det du/dv| = -(per-image sum of s) into
        sum_log_det_J: the mirror of forward_and_Jacobian (cnf_coupling_inverse_logdet)."""
        v = self._check(v, 'v')
        f = self._flow
        B = v.shape[0]
        u = torch.empty_like(v)
        ld = torch.zeros(B, device=v.device, dtype=torch.float32)
        ws = f._workspace(B)
        check(_lib.load().cnf_coupling_inverse_logdet(f._plan, self._layer, ptr(f.params), ptr(f._aux), ptr(v), ptr(u),
                                                      ptr(ld), ptr(ws), B, _stream()), 'cnf_coupling_inverse_logdet')
        return u, _accumulate_logdet(sum_log_det_J, ld), zy

    def gradients(self, u, dv, dlogdet=0.0):
        """Vector-Jacobian product of forward_and_Jacobian at u: (dL/du, dL/dparams) for
        dL/dv = dv and dL/d(per-image log-det) = dlogdet (the training backward of this layer;
        dparams is the flat canonical vector, zero outside this layer's parameters)."""
        u = self._check(u, 'u')
        dv = self._check(dv, 'dv')
        f = self._flow
        B = u.shape[0]
        du = torch.empty_like(u)
        dp = torch.empty(f.num_params, device=u.device, dtype=torch.float32)
        ws = f._train_workspace(B)
        check(_lib.load().cnf_coupling_backward(f._plan, self._layer, ptr(f.params), ptr(u), ptr(dv), ptr(du),
                                                float(dlogdet), ptr(ws), B, ptr(dp), _stream()),
              'cnf_coupling_backward')
        return du, dp


# ---------------------------------------------------------------------------------------------
# metrics (keras.metrics.Mean stand-in, :1692-1718)
# ---------------------------------------------------------------------------------------------

class Mean:
    """keras.metrics.Mean (the loss trackers of :1454-1457): the running mean of update_state values.
    Fed device tensors (train_step / test_step) it accumulates on the device in float64 — the same
    double arithmetic as a host float sum — and result() is a 0-d device tensor, as TF's train_step
    returns tensors: no host read per step (the fit loop reads the epoch's values once, at its end)."""
    def __init__(self, name):
        self.name = name
        self.reset_state()

    def reset_state(self):
        self.total = 0.0
        self.count = 0

    def update_state(self, v):
        if isinstance(v, torch.Tensor):
            v = v.detach().to(torch.float64)
        else:
            v = float(v)
        self.total = self.total + v
        self.count += 1

    def result(self):
        """Always a 0-d float64 tensor (on the device the values came from; a CPU zero before any update)."""
        if not self.count:
            return torch.zeros((), dtype=torch.float64)
        return torch.as_tensor(self.total / self.count, dtype=torch.float64)


# ---------------------------------------------------------------------------------------------
# cFlow
# ---------------------------------------------------------------------------------------------

class cFlow:
    """Conditional multi-scale RealNVP (conv_cINN_make_model.py:1408-1904) on MI355X.

    Extra keyword arguments (not in the reference): `group_mode` ('reference' reproduces the
    late-bound Lambda closure of conv_cINN_base_functions.py:402, 'intended' the textbook
    grouped convolution), `device`, `seed` (parameter init), `debug_options` (a dict or a
    "NAME=V,..." string selecting the alternative code paths the parity tests compare against:
    include/cnf.h cnf_flow_desc.debug_options; None = the defaults, which are what is benchmarked)."""

    def __init__(self, io_shape, x_d, squeeze_factor_block_list, ResNeXt_block_list, num_kernels_list,
                 cardinality_list, lambda_y=100, ksize=3, LAYER_NORM=True, DILATIONS=True, init=None,
                 group_mode='reference', device=None, seed=0, debug_options=None):
        lib = _lib.load()
        self.io_shape = [int(v) for v in io_shape]
        self.x_d = int(x_d)
        self.squeeze_factor_block_list = list(squeeze_factor_block_list)
        self.ResNeXt_block_list = list(ResNeXt_block_list)
        self.num_kernels_list = list(num_kernels_list)
        self.cardinality_list = list(cardinality_list)
        self.lambda_y = float(lambda_y)
        self.ksize = int(ksize)
        self.LAYER_NORM = bool(LAYER_NORM)
        self.DILATIONS = bool(DILATIONS)
        self.init = init
        if group_mode not in GROUP_MODES:
            raise ValueError(f'group_mode must be one of {list(GROUP_MODES)}')
        self.group_mode = group_mode
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())

        nb = len(self.squeeze_factor_block_list)
        assert nb == len(self.ResNeXt_block_list) == len(self.num_kernels_list) == len(self.cardinality_list), \
            'squeeze_factor_block_list, ResNeXt_block_list, num_kernels_list, and cardinality_list must all have the same length.'
        arr = lambda v: (C.c_int * len(v))(*[int(x) for x in v])
        self._keep = [arr(self.squeeze_factor_block_list), arr(self.ResNeXt_block_list),
                      arr(self.num_kernels_list), arr(self.cardinality_list)]
        desc = _lib.cnf_flow_desc(self.io_shape[0], self.io_shape[1], self.io_shape[2], self.x_d, nb,
                                  self._keep[0], self._keep[1], self._keep[2], self._keep[3],
                                  self.lambda_y, self.ksize, int(self.LAYER_NORM), int(self.DILATIONS),
                                  GROUP_MODES[group_mode])
        if isinstance(debug_options, dict):
            debug_options = ','.join(f'{k}={int(v)}' for k, v in debug_options.items())
        self.debug_options = debug_options or ''
        # a flow the kernels cannot run fails here, like the reference's asserts, in either group mode
        # (through the C ABI an 'intended' plan is not dry-run by default: include/cnf.h)
        opts = self.debug_options
        if 'SCHEDULE_CHECK' not in opts:
            opts = (opts + ',' if opts else '') + 'SCHEDULE_CHECK=1'
        self._opts_buf = C.create_string_buffer(opts.encode())
        desc.debug_options = C.cast(self._opts_buf, C.c_char_p)
        plan = C.c_void_p()
        check(lib.cnf_plan_create(C.byref(desc), C.byref(plan)), 'cFlow')
        self._plan = plan

        # parameter table
        self.param_specs = []
        name = C.create_string_buffer(256)
        off = C.c_int64()
        nd = C.c_int()
        shp = (C.c_int * 4)()
        for i in range(lib.cnf_plan_num_param_tensors(plan)):
            check(lib.cnf_plan_param_tensor(plan, i, name, 256, C.byref(off), C.byref(nd), shp), 'param table')
            self.param_specs.append((name.value.decode(), int(off.value), tuple(shp[j] for j in range(nd.value))))
        self._param_index = {n: (o, s) for n, o, s in self.param_specs}
        self.num_params = int(lib.cnf_plan_num_params(plan))
        self.params = torch.empty(self.num_params, device=self.device, dtype=torch.float32)
        self._aux = torch.empty(int(lib.cnf_plan_aux_floats(plan)), device=self.device, dtype=torch.float32)
        self._ws = {}

        # layers_list / squeeze_factor_layers_list (:1630-1689)
        self.layers_list: List[Layer] = []
        self.squeeze_factor_layers_list: List[Layer] = []
        info = _lib.cnf_layer_info()
        for li in range(lib.cnf_plan_num_layers(plan)):
            check(lib.cnf_plan_layer_info(plan, li, C.byref(info)), 'layer info')
            if info.kind == 0:
                self.layers_list.append(coupling_layer(self, li, info))
            elif info.kind == 1:
                L = squeeze_layer()
                self.layers_list.append(L)
                self.squeeze_factor_layers_list.append(L)
            else:
                L = factor_out_zy_layer(info.num_prev_factors)
                self.layers_list.append(L)
                self.squeeze_factor_layers_list.append(L)
        self.u1_mask_indices = [[0, 1, 2, 3] for _ in range(nb)]
        self.num_coupling_blocks = nb

        self.loss_tracker = Mean('loss')
        self.z_loss_tracker = Mean('z_loss')
        self.y_loss_tracker = Mean('y_loss')
        self.detJ_loss_tracker = Mean('detJ_loss')

        self.set_weights(self.initial_weights(seed))

    # -- lifecycle ------------------------------------------------------------------------------
    def __del__(self):
        try:
            if getattr(self, '_plan', None):
                _lib.load().cnf_plan_destroy(self._plan)
                self._plan = None
        except Exception:
            pass

    # -- parameters -----------------------------------------------------------------------------
    def initial_weights(self, seed=0) -> np.ndarray:
        """Reference initialisers: Conv2D kernels Orthogonal(gain=0.1) (:1442), biases 0,
        LayerNorm gamma 1 / beta 0, tanh scale 1 (:109-112)."""
        rng = np.random.default_rng(seed)
        flat = np.empty(self.num_params, dtype=np.float32)
        for n, o, s in self.param_specs:
            size = int(np.prod(s)) if s else 1
            if n.endswith('.kernel'):
                rows = int(np.prod(s[:-1]))
                cols = s[-1]
                a = rng.standard_normal((max(rows, cols), min(rows, cols)))
                q, r = np.linalg.qr(a)
                q = q * np.sign(np.diag(r))
                if rows < cols:
                    q = q.T
                v = 0.1 * q.reshape(-1)
            elif n.endswith('.gamma') or n.endswith('.w'):
                v = np.ones(size)
            else:
                v = np.zeros(size)
            flat[o:o + size] = v
        return flat

    def set_weights(self, weights):
        """weights: flat canonical vector (numpy/torch) or {name: array} dict."""
        if isinstance(weights, dict):
            flat = np.empty(self.num_params, dtype=np.float32)
            for n, o, s in self.param_specs:
                size = int(np.prod(s)) if s else 1
                flat[o:o + size] = np.asarray(weights[n], dtype=np.float32).reshape(-1)
            weights = flat
        if isinstance(weights, np.ndarray):
            weights = torch.from_numpy(np.ascontiguousarray(weights, dtype=np.float32))
        if weights.numel() != self.num_params:
            raise ValueError(f'expected {self.num_params} parameters, got {weights.numel()}')
        self.params.copy_(weights.reshape(-1).to(self.device, torch.float32))
        check(_lib.load().cnf_pack_params(self._plan, ptr(self.params), ptr(self._aux), _stream()), 'pack params')

    def get_weights(self) -> Dict[str, np.ndarray]:
        flat = self.params.detach().cpu().numpy()
        return {n: flat[o:o + (int(np.prod(s)) if s else 1)].reshape(s) for n, o, s in self.param_specs}

    def get_param(self, name):
        o, s = self._param_index[name]
        size = int(np.prod(s)) if s else 1
        return self.params[o:o + size].reshape(s)

    @property
    def trainable_variables(self):
        return [self.get_param(n) for n, _, _ in self.param_specs]

    def _workspace(self, B):
        ws = self._ws.get(B)
        if ws is None:
            nbytes = int(_lib.load().cnf_plan_workspace_bytes(self._plan, B))
            ws = torch.empty(max(nbytes, 256), device=self.device, dtype=torch.uint8)
            self._ws[B] = ws
        return ws

    # -- metrics --------------------------------------------------------------------------------
    @property
    def metrics(self):
        return [self.loss_tracker, self.z_loss_tracker, self.y_loss_tracker, self.detJ_loss_tracker]

    # -- the hot path ---------------------------------------------------------------------------
    def call(self, uv, direction=-1, per_image_logdet=False, layerwise=False, noise=None, inverse_logdet=False):
        """cFlow.call (:1723-1798). direction=+1: xy -> (zy, log_detJ) with log_detJ the batch-mean
        scalar (a (B,) tensor with per_image_logdet=True); direction=-1: zy -> xy, or with
        inverse_logdet=True (xy, logdet) with logdet[B] = log|det d xy / d zy| per image, minus the sum of
        every coupling layer's s (cnf_flow_inverse_logdet; xy is the plain inverse's bit for bit).
        layerwise=True walks layers_list through the per-layer entry points exactly as the
        reference loop does; the default runs the whole schedule in one native call.
        noise=(alpha, seed, offset[, logit_a]) (direction=+1): the input prepared as the reference's
        training pipeline does (conv_cINN.py:246-315) -- the logit map of
        preprocess_dataset_class(LOGITS=True, a=logit_a) on the x channels when logit_a is given
        (conv_cINN_base_functions.py:174-231), then instance_noise(., alpha) (:635-654) -- inside
        the first coupling layer's gather (cnf_flow_forward_noise), returning (zy, log_detJ,
        xy_noisy); xy_noisy equals base_functions.instance_noise(xy', alpha, seed, offset) bit for
        bit (xy' = xy with its x channels through preprocess_dataset_class) and is the xy of the
        loss."""
        uv = _as_input(uv, 'uv')
        if tuple(uv.shape[1:]) != tuple(self.io_shape):
            raise ValueError(f'input shape {tuple(uv.shape)} != [None, {self.io_shape}]')
        B = uv.shape[0]
        if inverse_logdet and direction != -1:
            raise ValueError('inverse_logdet applies to direction=-1 only (direction=+1 returns its log-det already)')
        if noise is not None:
            if direction != 1:
                raise ValueError('noise applies to the forward direction only')
            alpha, seed, offset, logit_a = (tuple(noise) + (0, 0, 0.0))[:4]
            if layerwise:
                from .base_functions import instance_noise, preprocess_dataset_class
                xp = uv
                if logit_a:
                    xp = torch.cat([preprocess_dataset_class(uv[..., :self.x_d], LOGITS=True, a=logit_a),
                                    uv[..., self.x_d:]], dim=-1).contiguous()
                xn = instance_noise(xp, alpha, seed, offset)
                zy, ld = self._call_layerwise_forward(xn)
            else:
                xn = torch.empty_like(uv)
                zy = torch.empty_like(uv)
                ld = torch.empty(B, device=uv.device, dtype=torch.float32)
                ws = self._workspace(B)
                check(_lib.load().cnf_flow_forward_noise(self._plan, ptr(self.params), ptr(self._aux), ptr(uv),
                                                         float(logit_a), float(alpha), int(seed) & (2 ** 64 - 1),
                                                         int(offset) & (2 ** 64 - 1), ptr(xn), ptr(zy), ptr(ld),
                                                         ptr(ws), B, _stream()), 'cnf_flow_forward_noise')
            return zy, (ld if per_image_logdet else ld.mean()), xn
        if direction == 1:
            if layerwise:
                zy, ld = self._call_layerwise_forward(uv)
            else:
                zy = torch.empty_like(uv)
                ld = torch.empty(B, device=uv.device, dtype=torch.float32)
                ws = self._workspace(B)
                check(_lib.load().cnf_flow_forward(self._plan, ptr(self.params), ptr(self._aux), ptr(uv), ptr(zy),
                                                   ptr(ld), ptr(ws), B, _stream()), 'cnf_flow_forward')
            return zy, (ld if per_image_logdet else ld.mean())
        elif direction == -1:
            if layerwise:
                return self._call_layerwise_inverse(uv, inverse_logdet)
            xy = torch.empty_like(uv)
            ws = self._workspace(B)
            if inverse_logdet:
                ld = torch.empty(B, device=uv.device, dtype=torch.float32)
                check(_lib.load().cnf_flow_inverse_logdet(self._plan, ptr(self.params), ptr(self._aux), ptr(uv), ptr(xy),
                                                          ptr(ld), ptr(ws), B, _stream()), 'cnf_flow_inverse_logdet')
                return xy, ld
            check(_lib.load().cnf_flow_inverse(self._plan, ptr(self.params), ptr(self._aux), ptr(uv), ptr(xy),
                                               ptr(ws), B, _stream()), 'cnf_flow_inverse')
            return xy
        raise ValueError('direction must be +1 or -1')

    __call__ = call

    def _call_layerwise_forward(self, uv):
        B = uv.shape[0]
        log_detJ = torch.zeros(B, device=uv.device, dtype=torch.float32)
        zy = None
        for layer in self.layers_list:                          # :1748-1752
            uv, log_detJ, zy = layer.forward_and_Jacobian(uv, log_detJ, zy)
        if len(self.squeeze_factor_layers_list) == 0:           # :1755-1757
            return uv, log_detJ
        zy = _concat(zy, uv)                                    # :1762
        vu = None
        for layer in reversed(self.squeeze_factor_layers_list):  # :1767-1770
            vu, zy = layer.backward(vu, zy)
        return vu, log_detJ

    def _call_layerwise_inverse(self, uv, inverse_logdet=False):
        B = uv.shape[0]
        zy = None
        if self.squeeze_factor_layers_list:                     # :1782-1788
            for layer in self.squeeze_factor_layers_list:
                uv, _, zy = layer.forward_and_Jacobian(uv, None, zy)
        vu = uv
        if inverse_logdet:   # the couplings through backward_and_Jacobian; squeeze / factor layers have none
            ld = torch.zeros(B, device=uv.device, dtype=torch.float32)
            for layer in reversed(self.layers_list):
                if isinstance(layer, coupling_layer):
                    vu, ld, zy = layer.backward_and_Jacobian(vu, ld, zy)
                else:
                    vu, zy = layer.backward(vu, zy)
            return vu, ld
        for layer in reversed(self.layers_list):                # :1793-1796
            vu, zy = layer.backward(vu, zy)
        return vu

    # -- sampling -------------------------------------------------------------------------------
    def sample(self, y, num_samples, temperature=1.0, seed=0, offset=0, chunk=None, logit_a=None, residual=False,
               return_samples=True, return_stats=True, return_y_dev=False, return_log_prob=False, truth=None,
               hist=None, quantiles=None, return_sq_err=None):
        """num_samples draws of x given each condition y and their per-pixel statistics: the recipe of
        TOYcINN.py:807-817 (z from the prior, concat y, the model in the generative direction, :1774-1798)
        with the post-transforms and the reduction over the draws, in one native call (cnf_flow_sample).

        y: [B,H,W,D-x_d] on the device, or [H,W,D-x_d] for one condition. The latent of condition b, draw s
        is temperature * renew_noise of a [B,S,H,W,x_d] tensor at (seed, offset); every drawn x goes through
        de_logitify(., logit_a) when logit_a is given, then + y when residual (RESIDUAL=True super-resolution:
        needs D - x_d == x_d). The B*S images run through the inverse `chunk` at a time (default
        min(B*S, 64)); no result depends on chunk, bit for bit.

        Returns a dict with the requested ones of 'samples' [B,S,H,W,x_d], 'mean' and 'std' [B,H,W,x_d]
        (over the draws, population form: np.std) and 'y_dev' [B,S] (sum |y_hat - y| of each draw: how
        well it honours its condition). With return_samples=False no [B,S,...] tensor is allocated.
        return_log_prob=True adds 'log_prob' [B,S]: the model's log-density of each draw in the flow's input
        space (before de_logitify / residual), llz + the sum of every coupling's s, i.e. what nll_sums reports
        as llz + logdet for that draw's (xy_hat, zy) -- from the inverse's own s (cnf_flow_sample_logp), for
        ranking the draws of a condition, importance weights or typicality checks. It may be the only output.

        Scoring the draws in the same call, without the [B,S,...] tensor (cnf_flow_sample_score; with none of
        these arguments the call is the one above):
        truth [B,H,W,x_d] (or [H,W,x_d]), in the space of the returned samples (after de_logitify and the
        residual), adds 'rank' (int32 [B,H,W,x_d]: how many of the S draws lie below the truth; uniform on
        0..S for a calibrated model), 'abs_err' ([B,H,W,x_d]: the mean |draw - truth|) and 'sq_err' ([B,S]:
        the sum over the image of (draw - truth)^2, i.e. which draw is closest; return_sq_err=False leaves it out).
        hist=(bins, lo, hi), 2 <= bins <= 256, adds 'hist' (int32 [B,H,W,x_d,bins]: the draws per bin of
        [lo, hi); draws outside are not counted) and 'hist_centers' [bins].
        quantiles=(0.05, 0.5, 0.95) (up to 8 levels in [0, 1]; needs hist) adds 'quantiles' [Q,B,H,W,x_d], read
        off the histogram by interpolation inside a bin: within one bin width of the draws' own quantile, NaN
        where no draw fell into [lo, hi). Like everything else here they do not depend on chunk, bit for bit."""
        y = _as_input(y, 'y')
        H, W, D = self.io_shape
        if y.dim() == 3:
            y = y.unsqueeze(0)
        if tuple(y.shape[1:]) != (H, W, D - self.x_d):
            raise ValueError(f'y has shape {tuple(y.shape)}, expected [None, {H}, {W}, {D - self.x_d}]')
        B, S = int(y.shape[0]), int(num_samples)
        if chunk is None:
            chunk = max(1, min(B * S, 64))
        desc = _lib.cnf_sample_desc(S, int(chunk), float(temperature), int(seed) & (2 ** 64 - 1),
                                    int(offset) & (2 ** 64 - 1), float(logit_a or 0.0), int(bool(residual)))
        lib = _lib.load()
        key = ('sample', B, S, int(chunk))
        ws = _call_workspace(self._ws, key, self.device, 'cFlow.sample',
                             lambda: lib.cnf_plan_sample_workspace_bytes(self._plan, B, C.byref(desc)))

        def new(*shape):
            return torch.empty(shape, device=y.device, dtype=torch.float32)
        out = {}
        if return_samples:
            out['samples'] = new(B, max(S, 0), H, W, self.x_d)
        if return_stats:
            out['mean'], out['std'] = new(B, H, W, self.x_d), new(B, H, W, self.x_d)
        if return_y_dev:
            out['y_dev'] = new(B, max(S, 0))
        if truth is not None or hist is not None or quantiles is not None:
            if return_log_prob:
                out['log_prob'] = new(B, max(S, 0))
            return self._sample_score(y, desc, ws, out, truth, hist, quantiles, return_sq_err)
        if return_log_prob:
            out['log_prob'] = new(B, max(S, 0))
            check(lib.cnf_flow_sample_logp(self._plan, ptr(self.params), ptr(self._aux), ptr(y), C.byref(desc),
                                           ptr(out.get('samples')), ptr(out.get('mean')), ptr(out.get('std')),
                                           ptr(out.get('y_dev')), ptr(out['log_prob']), ptr(ws), B, _stream()),
                  'cnf_flow_sample_logp')
            return out
        check(lib.cnf_flow_sample(self._plan, ptr(self.params), ptr(self._aux), ptr(y), C.byref(desc),
                                  ptr(out.get('samples')), ptr(out.get('mean')), ptr(out.get('std')),
                                  ptr(out.get('y_dev')), ptr(ws), B, _stream()),
              'cnf_flow_sample')
        return out

    def _sample_score(self, y, desc, ws, out, truth, hist, quantiles, return_sq_err):
        """sample()'s call with a truth, a histogram box or quantile levels (cnf_flow_sample_score): adds the
        score outputs to `out`, the dict of the plain outputs already allocated."""
        H, W, D = self.io_shape
        B = int(y.shape[0])
        sd, truth = _score_setup(out, (B, H, W, self.x_d), int(desc.num_samples), y.device, truth, hist, quantiles,
                                 return_sq_err)
        check(_lib.load().cnf_flow_sample_score(
            self._plan, ptr(self.params), ptr(self._aux), ptr(y), C.byref(desc), C.byref(sd), ptr(truth),
            ptr(out.get('samples')), ptr(out.get('mean')), ptr(out.get('std')), ptr(out.get('y_dev')),
            ptr(out.get('log_prob')), ptr(out.get('rank')), ptr(out.get('abs_err')), ptr(out.get('sq_err')),
            ptr(out.get('hist')), ptr(out.get('quantiles')), ptr(ws), B, _stream()), 'cnf_flow_sample_score')
        return out

    # -- density of given images ----------------------------------------------------------------
    def log_prob(self, x, y, logit_a=None, residual=False, chunk=None, pairwise=None, return_terms=False,
                 log_prior=None, return_posterior=False):
        """The model's log-density of given images, per condition: sample()'s counterpart, in one native call
        (cnf_flow_log_prob).

        x: [B,H,W,x_d] on the device (or [H,W,x_d] for one image), in the space of sample()'s 'samples': after
        de_logitify(., logit_a) when logit_a is given and after + y when residual. y: [B,H,W,D-x_d], image b
        under its own condition (paired), or with pairwise=True [K,H,W,D-x_d], every image under every condition
        ([H,W,D-x_d]: one condition). pairwise=None means paired when the leading dimensions agree and raises
        otherwise. The pairs run through the forward `chunk` at a time (default min(pairs, 64)); no result
        depends on chunk, bit for bit, and the pairwise call equals the paired one on the expanded pairs.

        Returns a dict, every entry [B] (paired) or [B,K] (pairwise):
        'log_prob' = llz + logdet + log_jac, the log-density of x given y in the space x lives in (sample()'s
        'log_prob' is the same quantity before de_logitify / the residual: it lacks log_jac);
        'bits_per_dim' = -log_prob / (H W x_d ln 2);
        with return_terms 'llz' and 'logdet' (what nll_sums reports for the flow-space image of x), 'log_jac'
        (the log-Jacobian of the logit map over the image; 0 without logit_a) and 'y_dev' (sum |y_hat - y|);
        with return_posterior (pairwise only) 'posterior' [B,K] = softmax_k(log_prob + log_prior), log_prior [K]
        or None for a uniform prior, and 'log_evidence' [B], the row's log-sum-exp.
        An image with an element outside the logit map's domain has log_prob -inf (and NaN llz, logdet,
        y_dev) under every condition; the other images are untouched."""
        x, y = _as_input(x, 'x'), _as_input(y, 'y')
        H, W, D = self.io_shape
        x_d = self.x_d
        if x.dim() == 3:
            x = x.unsqueeze(0)
        if y.dim() == 3:
            y = y.unsqueeze(0)
        if tuple(x.shape[1:]) != (H, W, x_d):
            raise ValueError(f'x has shape {tuple(x.shape)}, expected [None, {H}, {W}, {x_d}]')
        if tuple(y.shape[1:]) != (H, W, D - x_d):
            raise ValueError(f'y has shape {tuple(y.shape)}, expected [None, {H}, {W}, {D - x_d}]')
        B = int(x.shape[0])
        if pairwise is None:
            if int(y.shape[0]) != B:
                raise ValueError(f'x holds {B} images and y {int(y.shape[0])} conditions: pass pairwise=True to '
                                 f'score every image under every condition')
            pairwise = False
        if not pairwise and int(y.shape[0]) != B:
            raise ValueError(f'paired mode needs one condition per image: x holds {B}, y {int(y.shape[0])}')
        K = int(y.shape[0]) if pairwise else 0
        N = B * K if pairwise else B
        shape = (B, K) if pairwise else (B,)
        if (return_posterior or log_prior is not None) and not pairwise:
            raise AssertionError('cFlow.log_prob: the posterior over conditions needs pairwise=True')
        if log_prior is not None:
            return_posterior = True
            log_prior = _as_input(torch.as_tensor(log_prior, dtype=torch.float32, device=x.device), 'log_prior')
            if tuple(log_prior.shape) != (K,):
                raise ValueError(f'log_prior has shape {tuple(log_prior.shape)}, expected [{K}]')
        if chunk is None:
            chunk = max(1, min(N, 64))
        desc = _lib.cnf_logp_desc(K, int(chunk), float(logit_a or 0.0), int(bool(residual)))
        lib = _lib.load()
        key = ('log_prob', int(chunk))
        ws = _call_workspace(self._ws, key, self.device, 'cFlow.log_prob',
                             lambda: lib.cnf_plan_logp_workspace_bytes(self._plan, B, C.byref(desc)))

        def new(*s):
            return torch.empty(s, device=x.device, dtype=torch.float32)
        out = {'log_prob': new(*shape)}
        if return_terms:
            for n in ('llz', 'logdet', 'log_jac', 'y_dev'):
                out[n] = new(*shape)
        if return_posterior:
            out['posterior'], out['log_evidence'] = new(B, K), new(B)
        check(lib.cnf_flow_log_prob(self._plan, ptr(self.params), ptr(self._aux), ptr(x), ptr(y), C.byref(desc),
                                    ptr(out['log_prob']), ptr(out.get('llz')), ptr(out.get('logdet')),
                                    ptr(out.get('log_jac')), ptr(out.get('y_dev')), ptr(log_prior),
                                    ptr(out.get('posterior')), ptr(out.get('log_evidence')), ptr(ws), B, _stream()),
              'cnf_flow_log_prob')
        out['bits_per_dim'] = out['log_prob'] * (-1.0 / (H * W * x_d * math.log(2.0)))
        return out

    # -- input gradients of the log-density -------------------------------------------------------
    def _paired_xy(self, x, y, who):
        """x [B,H,W,x_d] and y [B,H,W,D-x_d] of a paired call ([H,W,.]: one image), checked as log_prob's"""
        x, y = _as_input(x, 'x'), _as_input(y, 'y')
        H, W, D = self.io_shape
        if x.dim() == 3:
            x = x.unsqueeze(0)
        if y.dim() == 3:
            y = y.unsqueeze(0)
        if tuple(x.shape[1:]) != (H, W, self.x_d):
            raise ValueError(f'x has shape {tuple(x.shape)}, expected [None, {H}, {W}, {self.x_d}]')
        if tuple(y.shape[1:]) != (H, W, D - self.x_d):
            raise ValueError(f'y has shape {tuple(y.shape)}, expected [None, {H}, {W}, {D - self.x_d}]')
        if int(y.shape[0]) != int(x.shape[0]):
            raise ValueError(f'{who} needs one condition per image: x holds {int(x.shape[0])}, y {int(y.shape[0])}')
        return x, y

    def score(self, x, y, logit_a=None, residual=False, chunk=None, return_grad_y=False):
        """The gradient of the log-density with respect to the image and to the condition, in one native call
        (cnf_flow_score): the exact derivative of log_prob(x, y, logit_a, residual)['log_prob'] (paired: image
        b under condition b) as a function of x and of y.

        x: [B,H,W,x_d], y: [B,H,W,D-x_d] on the device (or [H,W,.] for one image), as log_prob takes them. The
        images run `chunk` at a time (default min(B, 64)) through the training forward and a backward that
        computes data gradients only: no weight gradient is launched and no parameter gradient leaves it.

        Returns a dict: 'grad_x' [B,H,W,x_d] = d log_prob[b] / d x[b]; 'log_prob' [B]; with return_grad_y
        'grad_y' [B,H,W,D-x_d] = d log_prob[b] / d y[b] (through the condition channels of the flow's input and,
        with residual, through x - y): the sensitivity of this reconstruction's density to its condition.
        'log_prob' is independent of chunk, bit for bit. The gradients are equal across chunk only up to fp32
        rounding: a streamed layer's data-gradient convolution (launch_tconv, k_tconv_band) picks its tile height
        by the launch's workgroup count, which counts the chunk's images, and the tiles of an image are the fp64
        partials its fused LayerNorm-backward reduction sums. (The LayerNorm backward's own batch slices touch
        the gamma / beta partials only.)
        An image with an element outside the logit map's domain has log_prob -inf and NaN gradients; the other
        images are untouched."""
        x, y = self._paired_xy(x, y, 'cFlow.score')
        H, W, D = self.io_shape
        B = int(x.shape[0])
        if chunk is None:
            chunk = max(1, min(B, 64))
        desc = _lib.cnf_score_desc(int(chunk), float(logit_a or 0.0), int(bool(residual)))
        lib = _lib.load()
        ws = _call_workspace(self._ws, ('score', int(chunk)), self.device, 'cFlow.score',
                             lambda: lib.cnf_plan_score_workspace_bytes(self._plan, B, C.byref(desc)))
        out = {'grad_x': torch.empty_like(x), 'log_prob': torch.empty(B, device=x.device, dtype=torch.float32)}
        if return_grad_y:
            out['grad_y'] = torch.empty_like(y)
        check(lib.cnf_flow_score(self._plan, ptr(self.params), ptr(self._aux), ptr(x), ptr(y), C.byref(desc),
                                 ptr(out['grad_x']), ptr(out.get('grad_y')), ptr(out['log_prob']), ptr(ws), B,
                                 _stream()), 'cnf_flow_score')
        return out

    def ascend(self, x, y, steps, lr=1e-2, beta_1=0.9, beta_2=0.999, epsilon=1e-7, logit_a=None, residual=False,
               chunk=None, state=None, return_state=False):
        """`steps` steps of Adam gradient ascent on the model's log-density from the images x, the conditions y
        held fixed, in one native call without a host synchronisation between the steps (cnf_flow_ascend): a
        most-probable reconstruction to put next to sample()'s mean, or the local refinement of a draw.

        It climbs sample(return_log_prob=True)'s 'log_prob', llz + logdet, as a function of the flow's input:
        x is taken into that space as log_prob does (- y when residual, the logit map when logit_a is given),
        the ascent moves the x channels there, and the result comes back through sample()'s post-transforms.
        The mode of a density depends on the parametrisation: with logit_a the iterate approaches a mode of the
        density over the flow's (unconstrained) input space, in which the model was trained, and that is not the
        mode of the density over pixel space, which log_prob()'s 'log_prob' (with its log_jac term) describes.

        Returns a dict: 'x' [B,H,W,x_d], the last iterate in the space of x; 'log_prob' [steps+1,B], row t the
        flow-input-space log-density of iterate t (row 0: the start, the last row: 'x'); with return_state
        'state' = {'m', 'v' [B,H,W,x_d], 'step'}, Adam's moments and the steps taken, which passed back as
        state= continues the run: ascend(steps=a) then ascend(steps=b, state=...) from its 'x' equals
        ascend(steps=a + b) bit for bit when no transform is applied between them. The images run `chunk` at a
        time (default min(B, 64)); rows of 'log_prob' and iterates agree across chunk up to fp32 rounding (see
        score). An image with an element outside the logit map's domain keeps x and has -inf in every row."""
        x, y = self._paired_xy(x, y, 'cFlow.ascend')
        B = int(x.shape[0])
        steps = int(steps)
        if chunk is None:
            chunk = max(1, min(B, 64))
        first = 0
        m = v = None
        if state is not None:
            m, v, first = _as_input(state['m'], "state['m']"), _as_input(state['v'], "state['v']"), int(state['step'])
            if tuple(m.shape) != tuple(x.shape) or tuple(v.shape) != tuple(x.shape):
                raise ValueError(f"state['m'] and state['v'] must have x's shape {tuple(x.shape)}")
            m, v = m.clone(), v.clone()   # (the call updates them in place: the caller's state stays valid)
        elif return_state:
            m, v = torch.zeros_like(x), torch.zeros_like(x)
        desc = _lib.cnf_ascend_desc(int(chunk), steps, float(lr), float(beta_1), float(beta_2), float(epsilon),
                                    float(logit_a or 0.0), int(bool(residual)), first)
        lib = _lib.load()
        ws = _call_workspace(self._ws, ('ascend', int(chunk)), self.device, 'cFlow.ascend',
                             lambda: lib.cnf_plan_ascend_workspace_bytes(self._plan, B, C.byref(desc)))
        out = {'x': torch.empty_like(x),
               'log_prob': torch.empty((max(steps, 0) + 1, B), device=x.device, dtype=torch.float32)}
        check(lib.cnf_flow_ascend(self._plan, ptr(self.params), ptr(self._aux), ptr(x), ptr(y), C.byref(desc),
                                  ptr(out['x']), ptr(out['log_prob']), ptr(m), ptr(v), ptr(ws), B, _stream()),
              'cnf_flow_ascend')
        if return_state:
            out['state'] = {'m': m, 'v': v, 'step': first + steps}
        return out

    # -- loss -----------------------------------------------------------------------------------
    def nll_sums(self, xy, zy=None, logdet_per_image=None):
        """Per-batch sums of the NLL terms on device: (sum loss_i, sum -llz_i, sum -lly_i,
        sum -logdet_i) and the per-image (llz, lly, logdet) table."""
        xy = _as_input(xy, 'xy')
        B = xy.shape[0]
        if zy is None:
            zy, logdet_per_image = self.call(xy, 1, per_image_logdet=True)
        per = torch.empty((B, 3), device=xy.device, dtype=torch.float32)
        sums = torch.empty(4, device=xy.device, dtype=torch.float32)
        check(_lib.load().cnf_nll(self._plan, ptr(xy), ptr(zy), ptr(logdet_per_image), ptr(per), ptr(sums), B,
                                  _stream()), 'cnf_nll')
        return sums, per

    def log_loss(self, xy, process_group=None, noise=None):
        """cFlow.log_loss (:1800-1848): (loss, z_loss, y_loss, detJ_loss), batch means.
        With process_group given (True = the default group) and torch.distributed initialised,
        this rank's 4 sums and its image count are all-reduced (one collective of 5 fp32,
        distributed.reduce_nll_sums) so the means are over the global batch; shards may be
        ragged. noise=(alpha, seed, offset): the loss of the instance-noised input (call(noise=...):
        the noise applied inside the forward's first kernel, y' taken from the noisy input)."""
        from .distributed import reduce_nll_sums
        xy = _as_input(xy, 'xy')
        if noise is not None:
            zy, ld, xn = self.call(xy, 1, per_image_logdet=True, noise=noise)
            sums, _ = self.nll_sums(xn, zy, ld)
        else:
            sums, _ = self.nll_sums(xy)
        grp = None if process_group is True else process_group
        return reduce_nll_sums(sums, xy.shape[0], group=grp, all_reduce=process_group is not None)

    # -- training -------------------------------------------------------------------------------
    def compile(self, optimizer=None):
        """keras Model.compile(optimizer=Adam(...)) (conv_cINN.py:567-569)."""
        from .optimizers import Adam
        self.optimizer = optimizer if optimizer is not None else Adam()
        if hasattr(self.optimizer, 'bind'):   # the tensor table of the per-tensor clipping (optimizers.Adam.bind)
            self.optimizer.bind([o for _, o, _ in self.param_specs] + [self.num_params], self.device)

    def _train_workspace(self, B):
        key = ('train', B)
        ws = self._ws.get(key)
        if ws is None:
            nbytes = int(_lib.load().cnf_plan_train_workspace_bytes(self._plan, B))
            if nbytes <= 0:
                raise RuntimeError(_lib.load().cnf_last_error().decode())
            ws = torch.empty(nbytes, device=self.device, dtype=torch.uint8)
            self._ws[key] = ws
        return ws

    def _coupling_param_ranges(self):
        """{coupling index: (lo, hi)} of its parameters (names 'c<i>.*') in the flat canonical vector."""
        r = getattr(self, '_cranges', None)
        if r is None:
            r = {}
            for n, o, s in self.param_specs:
                ci = int(n.split('.', 1)[0][1:])
                size = int(np.prod(s)) if s else 1
                lo, hi = r.get(ci, (o, o))
                if o != hi:
                    raise RuntimeError(f'parameters of coupling {ci} are not contiguous')
                r[ci] = (lo, o + size)
            self._cranges = r
        return r

    def gradients(self, xy, process_group=None, overlap=None):
        """tape.gradient(loss, trainable_variables) of train_step (:1863-1869) as one flat
        vector in the canonical parameter order, plus the 4 loss terms (batch means, device
        scalars). With process_group (True = default group) the loss sums and the gradient are
        all-reduced, so both are those of the global batch: the 5-float loss all-reduce runs
        between forward and backward with no host read of its result (the backward takes the
        global image count from the device buffer), and each coupling layer's gradient range is
        all-reduced asynchronously as soon as that layer's backward is enqueued, overlapping the
        backward of the layers before it (the default on RCCL; overlap=False / True forces it off / on)."""
        from .distributed import allreduce_grads, pack_nll_sums
        xy = _as_input(xy, 'xy')
        if tuple(xy.shape[1:]) != tuple(self.io_shape):
            raise ValueError(f'input shape {tuple(xy.shape)} != [None, {self.io_shape}]')
        lib = _lib.load()
        B = xy.shape[0]
        ws = self._train_workspace(B)
        zy = torch.empty_like(xy)
        ld = torch.empty(B, device=xy.device, dtype=torch.float32)
        check(lib.cnf_flow_forward_train(self._plan, ptr(self.params), ptr(self._aux), ptr(xy), ptr(zy), ptr(ld),
                                         ptr(ws), B, _stream()), 'cnf_flow_forward_train')
        sums, _ = self.nll_sums(xy, zy, ld)
        buf = pack_nll_sums(sums, B)
        grp = None if process_group is True else process_group
        dist = None
        if process_group is not None:
            import torch.distributed as tdist
            if tdist.is_available() and tdist.is_initialized():
                dist = tdist
        if dist is not None:
            dist.all_reduce(buf, group=grp)
        if getattr(self, '_grads', None) is None or self._grads.numel() != self.num_params:
            self._grads = torch.empty(self.num_params, device=self.device, dtype=torch.float32)
        # the per-layer asynchronous all-reduce overlaps on RCCL (stream-ordered); gloo copies every range
        # through the host with a device sync per call, which the measured 1-GPU 2-rank rehearsal ran 33x
        # slower than one all-reduce after the backward: overlap by default on 'nccl' only
        if overlap is None:
            overlap = dist is not None and dist.get_backend(grp) == 'nccl'
        overlap = bool(overlap) and dist is not None
        works = []
        errors = []
        reported = []
        if overlap:
            ranges = self._coupling_param_ranges()
            grads = self._grads

            def done(_user, ci):
                # an exception must not escape into C (ctypes would print it and return, and this rank
                # would silently skip the layer's all-reduce while the other ranks pair it with the next)
                try:
                    reported.append(ci)
                    lo, hi = ranges[ci]
                    works.append(dist.all_reduce(grads[lo:hi], group=grp, async_op=True))
                except BaseException as e:   # noqa: BLE001 -- re-raised below
                    errors.append(e)
            cb = _lib.LAYER_DONE_FN(done)
        else:
            cb = _lib.LAYER_DONE_FN()
        check(lib.cnf_flow_backward_ex(self._plan, ptr(self.params), ptr(xy), ptr(zy), ptr(ws), B, ptr(buf) + 16,
                                       ptr(self._grads), cb, None, _stream()), 'cnf_flow_backward_ex')
        if overlap and not errors and sorted(reported) != sorted(self._coupling_param_ranges()):
            errors.append(RuntimeError(f'layer_done reported couplings {sorted(reported)}, expected each of '
                                       f'{sorted(self._coupling_param_ranges())} once'))
        if errors:
            # this rank's collective sequence no longer matches the other ranks': raised before any wait
            # (a wait could hang); the caller decides whether to abort the process group
            raise RuntimeError('per-layer gradient all-reduce failed') from errors[0]
        for w in works:
            w.wait()
        if dist is not None and not overlap:
            allreduce_grads(self._grads, group=grp)
        m = buf[:4] / buf[4]
        return self._grads, (m[0], m[1], m[2], m[3])

    def train_step(self, xy, process_group=None, overlap=None):
        """cFlow.train_step (:1850-1880): NLL gradient (GradientTape), optimizer.apply_gradients,
        Mean trackers; returns {'loss', 'z_loss', 'y_loss', 'detJ_loss'} as 0-d device tensors (TF
        returns tensors too; float() reads one). Data-parallel with process_group: the loss sums and
        the gradient are all-reduced over the global batch."""
        if getattr(self, 'optimizer', None) is None:
            self.compile()
        grads, terms = self.gradients(xy, process_group, overlap)
        self.optimizer.apply_flat(self.params, grads)
        check(_lib.load().cnf_pack_params(self._plan, ptr(self.params), ptr(self._aux), _stream()), 'pack params')
        for t, v in zip(self.metrics, terms):   # device scalars: no host sync (the trackers stay on the device)
            t.update_state(v)
        return {t.name: t.result() for t in self.metrics}

    def test_step(self, xy, process_group=None):
        """:1882-1904 — loss without a weight update; updates the Mean trackers. With
        process_group the loss terms are global-batch means (log_loss), the same on every rank."""
        loss, lz, ly, ld = self.log_loss(xy, process_group=process_group)
        for t, v in zip(self.metrics, (loss, lz, ly, ld)):
            t.update_state(v)
        return {t.name: t.result() for t in self.metrics}


# ---------------------------------------------------------------------------------------------
# cascaded super-resolution
# ---------------------------------------------------------------------------------------------

class cFlowCascade:
    """Multi-level super-resolution at inference: cFlow models trained independently per level
    (conv_cINN.py:28-30, one for 'SR4,2', one for 'SR2,1'), chained. The up-scaled degraded image conditions
    the first flow; each of its draws, up-scaled with `up`, conditions the second; and so on for up to 4
    stages. Every stage has the same x_d and io_d = 2 x_d, and twice the height and width of the one before."""

    MAX_STAGES = 4

    def __init__(self, flows: Sequence[cFlow]):
        self.flows = list(flows)
        if not 1 <= len(self.flows) <= self.MAX_STAGES:
            raise ValueError(f'cFlowCascade: 1..{self.MAX_STAGES} stages, got {len(self.flows)}')
        for l, f in enumerate(self.flows, 1):
            H, W, D = f.io_shape
            if D != 2 * f.x_d:
                raise ValueError(f'cFlowCascade: stage {l}: io_shape {f.io_shape} needs io_d == 2 * x_d (x_d {f.x_d})')
            if l == 1:
                continue
            q = self.flows[l - 2]
            if f.x_d != q.x_d:
                raise ValueError(f'cFlowCascade: stage {l}: x_d {f.x_d} differs from stage {l - 1}\'s {q.x_d}')
            if [H, W] != [2 * q.io_shape[0], 2 * q.io_shape[1]]:
                raise ValueError(f'cFlowCascade: stage {l}: io_shape {f.io_shape} must be twice stage {l - 1}\'s '
                                 f'{q.io_shape} in height and width')
            if f.device != q.device:
                raise ValueError(f'cFlowCascade: stage {l}: device {f.device} differs from stage {l - 1}\'s {q.device}')
        self.device = self.flows[0].device
        self.x_d = self.flows[0].x_d
        self._ws = {}

    def default_offsets(self, B, num_samples, offset=0):
        """The stages' streams one after the other: offset_l = offset + sum_{k<l} B N_k H_k W_k x_d."""
        offs, N = [], 1
        for f, S in zip(self.flows, num_samples):
            offs.append(int(offset))
            N *= int(S)
            offset += B * N * f.io_shape[0] * f.io_shape[1] * self.x_d
        return offs

    def sample(self, y, num_samples, temperature=1.0, seed=0, offset=0, chunk=None, logit_a=None, residual=False,
               return_samples=True, return_stats=True, return_stage_stats=False, return_y_dev=False,
               return_block_dev=False, truth=None, hist=None, quantiles=None, return_sq_err=None):
        """The distribution of the final high-resolution images given the degraded input, in one native call
        (cnf_flow_sample_cascade). y: [B,H_1,W_1,x_d] (or [H_1,W_1,x_d]), `up` of the low-resolution image, as
        preprocess_dataset_SR puts it in the y channels; num_samples = (S_1, ..., S_L): every node of stage l - 1
        gets S_l children, so a condition has N_l = S_1 ... S_l nodes at stage l and N_L leaves.

        The one rule: a node's condition is `up` of what cFlow.sample would have returned for its parent (after
        de_logitify(., logit_a) and + y with residual, at every stage). The call equals, bit for bit, the chain
        f1.sample(y, S_1) -> up -> f2.sample(., S_2) -> ... with the stage offsets below, but keeps only one chunk
        of images per stage on the device: the tree is walked depth-first, `chunk` images per inverse call
        (default min(B N_L, 64)), and no result depends on chunk, bit for bit.
        temperature and offset: a scalar or one value per stage. A scalar offset places the stages' Philox streams
        one after the other (default_offsets): offset_l = offset + sum_{k<l} B N_k H_k W_k x_d.

        Returns a dict with the requested ones of: 'samples' [B,N_L,H_L,W_L,x_d] (the leaves, in node order:
        leaf g's parent is g // S_L); 'mean', 'std' [B,H_L,W_L,x_d] over a condition's leaves (the posterior mean
        and std of the high-resolution image); with return_stage_stats 'stage_mean', 'stage_std': lists of L
        tensors [B,H_l,W_l,x_d] over the N_l nodes of each stage; 'y_dev': a list of L tensors [B,N_l], cFlow.sample's
        y_dev of every node against its own condition; 'block_dev': a list of L tensors [B,N_l], the sum over 2x2
        pixel blocks and channels of |mean over the block of (value - condition)|, the reference's stated check
        that a super-resolved draw's blocks average back to its condition (conv_cINN.py:44), 0 when they do.
        truth [B,H_L,W_L,x_d], hist=(bins, lo, hi), quantiles=, return_sq_err: cFlow.sample's scores of the N_L
        leaves of each condition ('rank', 'abs_err', 'sq_err' [B,N_L], 'hist', 'hist_centers', 'quantiles')."""
        lib = _lib.load()
        L = len(self.flows)
        y = _as_input(y, 'y')
        H1, W1, _ = self.flows[0].io_shape
        x_d = self.x_d
        if y.dim() == 3:
            y = y.unsqueeze(0)
        if tuple(y.shape[1:]) != (H1, W1, x_d):
            raise ValueError(f'y has shape {tuple(y.shape)}, expected [None, {H1}, {W1}, {x_d}]')
        S = [int(s) for s in num_samples]
        if len(S) != L:
            raise ValueError(f'num_samples needs one entry per stage ({L}), got {len(S)}')
        B = int(y.shape[0])
        N = [max(int(np.prod(S[:l + 1])), 0) for l in range(L)]
        T = [float(t) for t in temperature] if isinstance(temperature, (list, tuple)) else [float(temperature)] * L
        offs = ([int(o) for o in offset] if isinstance(offset, (list, tuple))
                else self.default_offsets(B, [max(s, 0) for s in S], int(offset)))
        if len(T) != L or len(offs) != L:
            raise ValueError(f'temperature and offset: a scalar or one value per stage ({L})')
        if chunk is None:
            chunk = max(1, min(B * N[-1], 64))
        desc = _lib.cnf_cascade_desc()
        desc.num_stages, desc.chunk, desc.seed = L, int(chunk), int(seed) & (2 ** 64 - 1)
        desc.logit_a, desc.residual = float(logit_a or 0.0), int(bool(residual))
        for l in range(L):
            desc.num_samples[l], desc.temperature[l], desc.offset[l] = S[l], T[l], offs[l] & (2 ** 64 - 1)
        plans = (C.c_void_p * L)(*[f._plan.value for f in self.flows])
        key = (B, int(chunk))
        ws = _call_workspace(self._ws, key, self.device, 'cFlowCascade.sample',
                             lambda: lib.cnf_cascade_workspace_bytes(plans, B, C.byref(desc)))

        def new(*shape):
            return torch.empty(shape, device=y.device, dtype=torch.float32)

        def stage_shape(l):
            return (B,) + tuple(self.flows[l].io_shape[:2]) + (x_d,)
        out = {}
        HL, WL, _ = self.flows[-1].io_shape
        if return_samples:
            out['samples'] = new(B, N[-1], HL, WL, x_d)
        mean, std = [None] * L, [None] * L
        if return_stage_stats:
            mean, std = [new(*stage_shape(l)) for l in range(L)], [new(*stage_shape(l)) for l in range(L)]
            out['stage_mean'], out['stage_std'] = mean, std
        elif return_stats:
            mean[-1], std[-1] = new(*stage_shape(L - 1)), new(*stage_shape(L - 1))
        if return_stats:
            out['mean'], out['std'] = mean[-1], std[-1]
        y_dev, block_dev = [None] * L, [None] * L
        if return_y_dev:
            out['y_dev'] = y_dev = [new(B, N[l]) for l in range(L)]
        if return_block_dev:
            out['block_dev'] = block_dev = [new(B, N[l]) for l in range(L)]
        sd = None
        if truth is not None or hist is not None or quantiles is not None or return_sq_err:
            sd, truth = _score_setup(out, stage_shape(L - 1), N[-1], y.device, truth, hist, quantiles, return_sq_err)

        def ptrs(ts):
            return (C.c_void_p * L)(*[ptr(t) for t in ts])
        check(lib.cnf_flow_sample_cascade(
            plans, ptrs([f.params for f in self.flows]), ptrs([f._aux for f in self.flows]), ptr(y), C.byref(desc),
            None if sd is None else C.byref(sd), ptr(truth), ptr(out.get('samples')), ptr(out.get('rank')),
            ptr(out.get('abs_err')), ptr(out.get('sq_err')), ptr(out.get('hist')), ptr(out.get('quantiles')),
            ptrs(mean), ptrs(std), ptrs(y_dev), ptrs(block_dev), ptr(ws), B, _stream()), 'cnf_flow_sample_cascade')
        return out
