"""Drop-in replacement for the reference's `TOYcINN_make_model.cINN_affine` (BASELINE configs[0]).

Same constructor arguments, `call(u, direction=-1)` / `log_loss` / `compile` / `train_step` /
`test_step` / `metrics` semantics as TOYcINN_make_model.py:105-506, on torch tensors [B, 3] fp32 on the ROCm device; the
flow runs in libcnf_hip.so (k_toy, k_toy_bwd for the gradient, k_toy_sample for `sample`, k_toy_density for `log_prob` / `density`) through the C ABI. Note the toy's direction convention is the
reverse of cFlow's: -1 maps xy' -> zy (training direction, returns the per-sample log-det),
+1 maps zy -> xy'.

Parameters: per coupling network j (mask type j % 6), the b net then the A net, each Dense as
kernel [in][out] then bias [out] (oracle.toy_np.net_specs order / names `t{j}.{b|A}.d{k}.*`).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr
from .make_model import Mean, _as_input, _stream

MASK_U1 = {0: [0], 1: [1], 2: [2], 3: [0, 1], 4: [0, 2], 5: [1, 2]}


def _default_mask_indices(n: int, seed: int):
    """arange(n) shuffled within consecutive groups of 6 (:192-205; seeded here)."""
    rng = np.random.default_rng(seed)
    out = []
    for g in range(n // 6):
        blk = np.arange(6 * g, 6 * (g + 1))
        rng.shuffle(blk)
        out.extend(int(v) for v in blk)
    out.extend(range(6 * (n // 6), n))
    return out


def _parse_box(G, lo, hi, x_d, what):
    """(G, lo, hi) of a grid of G bins per component over [lo, hi): lo / hi scalars or one value per component,
    returned as tuples padded to two components (cnf_toy_sample_desc.hist_lo, cnf_toy_density_desc.lo)."""
    G = int(G)
    lo = tuple(float(v) for v in (lo if isinstance(lo, (tuple, list)) else (lo,) * x_d))
    hi = tuple(float(v) for v in (hi if isinstance(hi, (tuple, list)) else (hi,) * x_d))
    if len(lo) != x_d or len(hi) != x_d:
        raise ValueError(f'{what} lo / hi need one value per component ({x_d})')
    return G, lo + (0.0,) * (2 - x_d), hi + (0.0,) * (2 - x_d)


class cINN_affine:
    """TOYcINN_make_model.cINN_affine (:105-506)."""

    def __init__(self, io_shape, x_d, num_coupling_layers, intermediate_dims, num_layers, init=None,
                 mask_indices: Optional[Sequence[int]] = None, device=None, seed: int = 0):
        self.io_shape = int(io_shape)
        self.x_d = int(x_d)
        self.num_coupling_layers = int(num_coupling_layers)
        self.intermediate_dims = int(intermediate_dims)
        self.num_layers = int(num_layers)
        self.init = init   # stored, unused — as in the reference (:138)
        self.lambda_y = 100
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        self.mask_indices = list(mask_indices) if mask_indices else _default_mask_indices(num_coupling_layers, seed)
        self._order = (C.c_int * len(self.mask_indices))(*self.mask_indices)
        self._desc = _lib.cnf_toy_desc(self.io_shape, self.x_d, self.num_coupling_layers, self.intermediate_dims,
                                       self.num_layers, self._order, float(self.lambda_y))
        lib = _lib.load()
        n = lib.cnf_toy_num_params(C.byref(self._desc))
        if n < 0:
            raise AssertionError(lib.cnf_last_error().decode())
        self.num_params = int(n)
        self.params = torch.empty(self.num_params, device=self.device, dtype=torch.float32)
        self._init_weights(seed)
        self._ws = {}   # B -> (training workspace, gradient buffer)
        self.loss_tracker = Mean('loss')
        self.z_loss_tracker = Mean('z_loss')
        self.y_loss_tracker = Mean('y_loss')
        self.detJ_loss_tracker = Mean('detJ_loss')

    # -- parameters ----------------------------------------------------------------------------
    def param_specs(self):
        specs = []
        H, L = self.intermediate_dims, self.num_layers
        for j in range(self.num_coupling_layers):
            u1 = len(MASK_U1[j % 6])
            u2 = self.io_shape - u1
            for blk in ('b', 'A'):
                dims = [u1] + [H] * (L + 1) + [u2]
                for k in range(L + 2):
                    specs.append((f't{j}.{blk}.d{k}.kernel', (dims[k], dims[k + 1])))
                    specs.append((f't{j}.{blk}.d{k}.bias', (dims[k + 1],)))
        return specs

    def _init_weights(self, seed):
        """glorot_uniform kernels, zero biases (Keras Dense defaults)."""
        rng = np.random.default_rng(seed)
        flat = []
        for n, s in self.param_specs():
            if n.endswith('.kernel'):
                lim = math.sqrt(6.0 / (s[0] + s[1]))
                flat.append(rng.uniform(-lim, lim, s).reshape(-1))
            else:
                flat.append(np.zeros(s).reshape(-1))
        self.set_weights(np.concatenate(flat))

    def set_weights(self, weights):
        if isinstance(weights, dict):
            weights = np.concatenate([np.asarray(weights[n], np.float32).reshape(-1) for n, _ in self.param_specs()])
        w = torch.as_tensor(np.ascontiguousarray(weights, dtype=np.float32)) if isinstance(weights, np.ndarray) \
            else weights
        if w.numel() != self.num_params:
            raise ValueError(f'expected {self.num_params} parameters, got {w.numel()}')
        self.params.copy_(w.reshape(-1).to(self.device, torch.float32))

    def get_weights(self) -> Dict[str, np.ndarray]:
        flat = self.params.detach().cpu().numpy()
        out, o = {}, 0
        for n, s in self.param_specs():
            size = int(np.prod(s))
            out[n] = flat[o:o + size].reshape(s)
            o += size
        return out

    @property
    def metrics(self):
        return [self.loss_tracker, self.z_loss_tracker, self.y_loss_tracker, self.detJ_loss_tracker]

    # -- the flow --------------------------------------------------------------------------------
    def _run(self, u, direction, want_terms=False):
        u = _as_input(u, 'u')
        if u.dim() != 2 or u.shape[1] != self.io_shape:
            raise AssertionError(f'u must have shape (batch, {self.io_shape})')
        B = u.shape[0]
        v = torch.empty_like(u)
        ld = torch.empty(B, device=u.device, dtype=torch.float32) if direction == -1 else None
        per = torch.empty((B, 3), device=u.device, dtype=torch.float32) if want_terms else None
        check(_lib.load().cnf_toy_call(C.byref(self._desc), ptr(self.params), ptr(u), ptr(v),
                                       ptr(ld) if ld is not None else None,
                                       ptr(per) if per is not None else None, B, direction, _stream()),
              'cnf_toy_call')
        return v, ld, per

    def call(self, u, direction=-1):
        """(:237-417) direction -1: xy' -> (zy, log_detJ[B]); +1: zy -> (xy', 0)."""
        if direction not in (-1, 1):
            raise AssertionError('direction must be -1 or +1')
        v, ld, _ = self._run(u, direction)
        return v, (ld if direction == -1 else 0)

    __call__ = call

    def sample(self, y, num_samples, temperature=1.0, seed=0, offset=0, return_samples=True, return_stats=True,
               return_y_dev=False, hist=None):
        """num_samples draws of x given each condition y, their statistics and an optional histogram: what
        the toy driver does once training ends (TOYcINN.py:807-817: z from the prior, concatenate y,
        model(zy, direction=1); :823-... the cloud per condition) in one fused native call (cnf_toy_sample,
        k_toy_sample: no [B*S, 3] tensor exists anywhere).

        y: [B, 3 - x_d] on the device, or [3 - x_d] for one condition. The latent of condition b, draw s is
        temperature * the N(0, 1) stream cnf_instance_noise writes into a [B, S, x_d] tensor at (seed, offset).
        hist: None, or (G, lo, hi) with lo / hi scalars or one value per component: the draws counted on a grid
        of G bins per component over [lo, hi), bin = floor((v - lo) * (G / (hi - lo))) in fp32.

        Returns a dict with the requested ones of 'samples' [B, S, x_d], 'mean' and 'std' [B, x_d] (over the
        draws, population form: np.std), 'y_dev' [B, S] (sum |y_hat - y| of each draw) and 'hist' (int32 counts,
        [B, G] or [B, G, G] with component 0 major). With return_samples=False no [B, S, .] tensor is
        allocated. The draws agree with call(zy, +1) up to rounding, not bit for bit (the hidden layers run on
        the matrix cores); each draw's bits depend only on the weights, its y, seed, stream index and
        temperature."""
        y = _as_input(y, 'y')
        yd = self.io_shape - self.x_d
        if y.dim() == 1:
            y = y.unsqueeze(0)
        if y.dim() != 2 or y.shape[1] != yd:
            raise ValueError(f'y has shape {tuple(y.shape)}, expected [None, {yd}]')
        B, S, x_d = int(y.shape[0]), int(num_samples), self.x_d
        G, lo, hi = 0, (0.0, 0.0), (0.0, 0.0)
        if hist is not None:
            G, lo, hi = hist
            G, lo, hi = _parse_box(G, lo, hi, x_d, 'hist')
            if G < 1:
                raise AssertionError('cINN_affine.sample: hist needs at least one bin')
        desc = _lib.cnf_toy_sample_desc(S, float(temperature), int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1),
                                        G, (C.c_float * 2)(*lo), (C.c_float * 2)(*hi))
        lib = _lib.load()
        key = ('sample', B, S)
        ws = self._ws.get(key)
        if ws is None:
            nbytes = int(lib.cnf_toy_sample_workspace_bytes(C.byref(self._desc), B, C.byref(desc)))
            if nbytes <= 0:   # an argument error, as the reference's asserts
                raise AssertionError(f'cINN_affine.sample: {lib.cnf_last_error().decode()}')
            ws = self._ws[key] = torch.empty(nbytes, device=self.device, dtype=torch.uint8)

        def new(*shape, dtype=torch.float32):
            return torch.empty(shape, device=y.device, dtype=dtype)
        out = {}
        if return_samples:
            out['samples'] = new(B, S, x_d)
        if return_stats:
            out['mean'], out['std'] = new(B, x_d), new(B, x_d)
        if return_y_dev:
            out['y_dev'] = new(B, S)
        if hist is not None:
            out['hist'] = new(B, *([G] * x_d), dtype=torch.int32)
        check(lib.cnf_toy_sample(C.byref(self._desc), ptr(self.params), ptr(y), C.byref(desc), ptr(out.get('samples')),
                                 ptr(out.get('mean')), ptr(out.get('std')), ptr(out.get('y_dev')), ptr(out.get('hist')),
                                 ptr(ws), B, _stream()), 'cnf_toy_sample')
        return out

    def _density(self, y, x, desc, N, shape, return_y_dev, return_z, log_mass, who):
        """cnf_toy_density on y [B, 3 - x_d] and x [B, N, x_d] (or None: desc's grid); the per-point outputs
        reshaped to [B, *shape]."""
        lib = _lib.load()
        B, x_d = int(y.shape[0]), self.x_d
        key = ('density', B, N)
        ws = self._ws.get(key)
        if ws is None:
            nbytes = int(lib.cnf_toy_density_workspace_bytes(C.byref(self._desc), B, C.byref(desc)))
            if nbytes <= 0:   # an argument error, as the reference's asserts
                raise AssertionError(f'cINN_affine.{who}: {lib.cnf_last_error().decode()}')
            ws = self._ws[key] = torch.empty(nbytes, device=self.device, dtype=torch.uint8)
        out = {'log_prob': torch.empty((B, N), device=y.device, dtype=torch.float32)}
        if log_mass:
            out['log_mass'] = torch.empty(B, device=y.device, dtype=torch.float32)
        if return_y_dev:
            out['y_dev'] = torch.empty((B, N), device=y.device, dtype=torch.float32)
        if return_z:
            out['z'] = torch.empty((B, N, x_d), device=y.device, dtype=torch.float32)
        check(lib.cnf_toy_density(C.byref(self._desc), ptr(self.params), ptr(y), ptr(x), C.byref(desc),
                                  ptr(out['log_prob']), ptr(out.get('y_dev')), ptr(out.get('z')), ptr(out.get('log_mass')),
                                  ptr(ws), B, _stream()), 'cnf_toy_density')
        for n in ('log_prob', 'y_dev'):
            if n in out:
                out[n] = out[n].reshape(B, *shape)
        if 'z' in out:
            out['z'] = out['z'].reshape(B, *shape, x_d)
        return out

    def _condition(self, y):
        y = _as_input(y, 'y')
        yd = self.io_shape - self.x_d
        if y.dim() != 2 or y.shape[1] != yd:
            raise ValueError(f'y has shape {tuple(y.shape)}, expected [None, {yd}]')
        return y

    def log_prob(self, x, y, return_y_dev=False, return_z=False):
        """The flow's exact log-density at given points, in one fused native call (cnf_toy_density, k_toy_density:
        no [B*N, 3] tensor and no zy exist anywhere): log_prob = log N(z; 0, I) + log|det J| of xy -> zy, the llz +
        log_detJ of log_loss per point. Where the model returns the condition (y_hat = y, a trained model) this is
        log p(x | y).

        x: [B, N, x_d] with y [B, 3 - x_d], or x [N, x_d] with y [3 - x_d] (one condition; the leading dimension
        is squeezed on return). Returns log_prob [B, N], or with return_y_dev / return_z a dict of 'log_prob',
        'y_dev' [B, N] (sum |y_hat - y| of each point, as sample's) and 'z' [B, N, x_d] (the latent image).

        model.log_prob(model.sample(y, S)['samples'], y) is each draw's log-density (and its 'z' recovers the
        draw's latent up to rounding). The values agree with call(xy, -1) up to rounding, not bit for bit (the
        hidden layers run on the matrix cores); a point's bits depend only on the weights, its y and its
        coordinates."""
        x, y = _as_input(x, 'x'), _as_input(y, 'y')
        one = x.dim() == 2 and y.dim() == 1
        if one:
            x, y = x.unsqueeze(0), y.unsqueeze(0)
        y = self._condition(y)
        if x.dim() != 3 or x.shape[0] != y.shape[0] or x.shape[2] != self.x_d:
            raise ValueError(f'x has shape {tuple(x.shape)}, expected [{y.shape[0]}, None, {self.x_d}]')
        N = int(x.shape[1])
        desc = _lib.cnf_toy_density_desc(N, 0, (C.c_float * 2)(0.0, 0.0), (C.c_float * 2)(0.0, 0.0))
        out = self._density(y, x, desc, N, (N,), return_y_dev, return_z, False, 'log_prob')
        if one:
            out = {n: t[0] for n, t in out.items()}
        return out if (return_y_dev or return_z) else out['log_prob']

    def density(self, y, G, lo, hi, return_y_dev=False, return_z=False):
        """The flow's exact log-density of x given each condition y on a grid of G bins per component over
        [lo, hi): the heat map of p(x | y), evaluated at the centres of the bins of sample(hist=(G, lo, hi)) (the
        curve those counts converge to), in one fused native call (cnf_toy_density).

        y: [B, 3 - x_d] on the device, or [3 - x_d] for one condition. lo / hi: scalars or one value per component,
        as sample's hist. Returns a dict: 'log_prob' [B, G] or [B, G, G] (component 0 major, as 'hist'), 'log_mass'
        [B] = log(sum exp(log_prob) * the cell volume), the share of the density inside the box (about 0 for a
        trained model and a box that covers it), 'centers', a tuple of x_d fp32 tensors [G]: lo + (i + 0.5) *
        ((hi - lo) / G) in fp32, one multiply and then one add; and with return_y_dev / return_z 'y_dev' (shaped
        as 'log_prob') and 'z' [B, G(, G), x_d]. density(...) equals log_prob at the centres bit for bit."""
        y = _as_input(y, 'y')
        if y.dim() == 1:
            y = y.unsqueeze(0)
        y = self._condition(y)
        x_d = self.x_d
        G, lo, hi = _parse_box(G, lo, hi, x_d, 'density')
        if G < 1:
            raise AssertionError('cINN_affine.density: the grid needs at least one bin')
        desc = _lib.cnf_toy_density_desc(0, G, (C.c_float * 2)(*lo), (C.c_float * 2)(*hi))
        out = self._density(y, None, desc, G ** x_d, (G,) * x_d, return_y_dev, return_z, True, 'density')
        idx = np.arange(G, dtype=np.float32) + np.float32(0.5)
        centers = []
        for c in range(x_d):
            step = (np.float32(hi[c]) - np.float32(lo[c])) / np.float32(G)
            centers.append(torch.from_numpy((np.float32(lo[c]) + (idx * step).astype(np.float32)).astype(np.float32))
                           .to(y.device))
        out['centers'] = tuple(centers)
        return out

    def log_loss(self, xy, process_group=None):
        """(:419-451) -> (loss, -mean llz, -mean lly, -mean log_detJ); with process_group the 4 sums
        and the sample count are all-reduced (one 5-float collective)."""
        from .distributed import reduce_nll_sums
        xy = _as_input(xy, 'xy')
        _, _, per = self._run(xy, -1, want_terms=True)
        sums = torch.empty(4, device=xy.device, dtype=torch.float32)
        check(_lib.load().cnf_toy_nll_sums(ptr(per), ptr(sums), xy.shape[0], _stream()), 'cnf_toy_nll_sums')
        grp = None if process_group is True else process_group
        return reduce_nll_sums(sums, xy.shape[0], group=grp, all_reduce=process_group is not None)

    # -- training -------------------------------------------------------------------------------
    def compile(self, optimizer=None):
        """keras Model.compile(optimizer=Adam(1e-4)) (TOYcINN.py:213-304)."""
        from .optimizers import Adam
        self.optimizer = optimizer if optimizer is not None else Adam()
        if hasattr(self.optimizer, 'bind'):   # the tensor table of the per-tensor clipping (optimizers.Adam.bind)
            offsets = [0]
            for _, s in self.param_specs():
                offsets.append(offsets[-1] + int(np.prod(s)))
            self.optimizer.bind(offsets, self.device)

    def _train_workspace(self, B):
        """(training workspace, flat gradient buffer), cached per B."""
        cache = self._ws
        ws = cache.get(B)
        if ws is None:
            nbytes = int(_lib.load().cnf_toy_train_workspace_bytes(C.byref(self._desc), B))
            if nbytes <= 0:
                raise RuntimeError(_lib.load().cnf_last_error().decode())
            ws = (torch.empty(nbytes, device=self.device, dtype=torch.uint8),
                  torch.empty(self.num_params, device=self.device, dtype=torch.float32))
            cache[B] = ws
        return ws

    def gradients(self, xy, process_group=None):
        """tape.gradient(loss, trainable_variables) of train_step (:453-481) as one flat vector in
        the canonical parameter order, plus the 4 loss terms (batch means, device scalars). With
        process_group (True = the default group) the 4 loss sums and the sample count are all-reduced
        (one 5-float collective) between forward and backward, the backward scales by 1 / the global
        count, and the gradient is all-reduced after it: both are those of the global batch. (The C
        ABI takes inv_batch by value, so the data-parallel path reads the reduced count on the host,
        once per step; without a process group the step has no host read.)"""
        from .distributed import allreduce_grads, pack_nll_sums
        xy = _as_input(xy, 'xy')
        if xy.dim() != 2 or xy.shape[1] != self.io_shape:
            raise AssertionError(f'xy must have shape (batch, {self.io_shape})')
        lib = _lib.load()
        B = xy.shape[0]
        ws, grads = self._train_workspace(B)
        zy = torch.empty_like(xy)
        per = torch.empty((B, 3), device=xy.device, dtype=torch.float32)
        check(lib.cnf_toy_forward_train(C.byref(self._desc), ptr(self.params), ptr(xy), ptr(zy), ptr(per), ptr(ws),
                                        B, _stream()), 'cnf_toy_forward_train')
        sums = torch.empty(4, device=xy.device, dtype=torch.float32)
        check(lib.cnf_toy_nll_sums(ptr(per), ptr(sums), B, _stream()), 'cnf_toy_nll_sums')
        buf = pack_nll_sums(sums, B)
        grp = None if process_group is True else process_group
        dist = None
        if process_group is not None:
            import torch.distributed as tdist
            if tdist.is_available() and tdist.is_initialized():
                dist = tdist
        n_global = B
        if dist is not None:
            dist.all_reduce(buf, group=grp)
            n_global = int(round(float(buf[4])))   # the C ABI takes inv_batch by value
        check(lib.cnf_toy_backward(C.byref(self._desc), ptr(self.params), ptr(xy), ptr(zy), ptr(ws), B,
                                   1.0 / n_global, ptr(grads), _stream()), 'cnf_toy_backward')
        if dist is not None:
            allreduce_grads(grads, group=grp)
        m = buf[:4] / buf[4]
        return grads, (m[0], m[1], m[2], m[3])

    def train_step(self, xy, process_group=None):
        """cINN_affine.train_step (:453-481): NLL gradient (GradientTape), optimizer.apply_gradients,
        Mean trackers; returns {'loss', 'z_loss', 'y_loss', 'detJ_loss'} as 0-d device tensors (no host
        read in the step). Data-parallel with process_group: see gradients."""
        if getattr(self, 'optimizer', None) is None:
            self.compile()
        grads, terms = self.gradients(xy, process_group)
        self.optimizer.apply_flat(self.params, grads)
        for t, v in zip(self.metrics, terms):   # device scalars: the trackers stay on the device
            t.update_state(v)
        return {t.name: t.result() for t in self.metrics}

    def test_step(self, xy, process_group=None):
        """(:483-506) loss without a weight update; updates the Mean trackers. With process_group
        the loss terms are global-batch means (log_loss)."""
        vals = [t.item() for t in self.log_loss(xy, process_group=process_group)]
        for tr, v in zip(self.metrics, vals):
            tr.update_state(v)
        return {tr.name: tr.result() for tr in self.metrics}
