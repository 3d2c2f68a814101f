"""Keras-compatible Adam for the training step (conv_cINN.py:567-569
`model.compile(optimizer=tf.keras.optimizers.Adam(learning_rate=...))`).

The update runs on the device (k_adam through `cnf_adam_step`) over the flat canonical parameter
vector, with the moment buffers kept as two more flat fp32 vectors of the same size (288 GB of HBM
holds them next to every activation of the largest BASELINE configuration). Keras semantics:
    m += (g - m)(1 - beta_1);  v += (g^2 - v)(1 - beta_2)
    p -= lr sqrt(1 - beta_2^t) / (1 - beta_1^t) * m / (sqrt(v) + epsilon)

The Keras clipping and averaging arguments (clipvalue, clipnorm, global_clipnorm, use_ema /
ema_momentum) and skip_nonfinite (a step whose gradient holds a NaN or an infinity changes nothing
and is counted) select the guarded step, `cnf_optim_step` (include/cnf.h states its rules): three
launches, the step count kept on the device, no host read anywhere. It clips per parameter tensor,
so it needs the model's tensor offsets: `cFlow.compile` / `cINN_affine.compile` hand them over
through `bind`. With none of these arguments set, apply_flat is the plain `cnf_adam_step` call.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr


def _clip_arg(name, value):
    """None (off) or a finite number > 0, as float (0.0 = off)"""
    if value is None:
        return 0.0
    value = float(value)
    if not math.isfinite(value) or value <= 0.0:
        raise ValueError(f'{name} must be a finite number > 0 (or None), got {value}')
    return value


class Adam:
    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, clipnorm=None, clipvalue=None,
                 global_clipnorm=None, use_ema=False, ema_momentum=0.99, skip_nonfinite=False):
        self.learning_rate = float(learning_rate)
        self.beta_1 = float(beta_1)
        self.beta_2 = float(beta_2)
        self.epsilon = float(epsilon)
        self.clipnorm = _clip_arg('clipnorm', clipnorm)
        self.clipvalue = _clip_arg('clipvalue', clipvalue)
        self.global_clipnorm = _clip_arg('global_clipnorm', global_clipnorm)
        if self.clipnorm and self.global_clipnorm:
            raise ValueError('clipnorm and global_clipnorm exclude each other (as in Keras): give one of them')
        self.use_ema = bool(use_ema)
        self.ema_momentum = float(ema_momentum)
        if self.use_ema and not 0.0 < self.ema_momentum < 1.0:
            raise ValueError(f'ema_momentum must be in (0, 1), got {ema_momentum}')
        self.skip_nonfinite = bool(skip_nonfinite)
        self.iterations = 0   # apply_flat calls (the guarded step's own counters: steps_applied, steps_skipped)
        self._m = None
        self._v = None
        self._ema = None
        self._offsets = None  # the model's tensor offsets [T + 1] (bind)
        self._dev = None      # the guarded step's device state (table, counters, stats, scales, workspace)

    @property
    def guarded(self) -> bool:
        """any option of the guarded step (cnf_optim_step) is set"""
        return bool(self.clipnorm or self.clipvalue or self.global_clipnorm or self.use_ema or self.skip_nonfinite)

    def bind(self, offsets, device=None):
        """The model's parameter table: offsets[T + 1] of its tensors in the flat vector (0 ... n,
        non-decreasing). The guarded step builds its slab table from them and uploads it here, once."""
        self._offsets = [int(o) for o in offsets]
        self._dev = None
        if self.guarded and device is not None:
            self._device_state(torch.device(device))

    def _device_state(self, device):
        if self._dev is not None and self._dev['device'] == device:
            return self._dev
        if self._offsets is None:
            raise RuntimeError('Adam with clipnorm / clipvalue / global_clipnorm / use_ema / skip_nonfinite works per '
                               'parameter tensor and has no tensor table: compile the model with it (cFlow.compile, '
                               'cINN_affine.compile) or call bind(offsets) first')
        lib = _lib.load()
        T = len(self._offsets) - 1
        n = self._offsets[-1] if self._offsets else 0
        offs = (C.c_int64 * (T + 1))(*self._offsets)
        nbytes = int(lib.cnf_optim_table_bytes(n, offs, T))
        if nbytes == 0:
            raise ValueError(lib.cnf_last_error().decode())
        host = np.zeros(nbytes, np.uint8)
        check(lib.cnf_optim_table_build(n, offs, T, host.ctypes.data), 'cnf_optim_table_build')
        num_slabs = int(lib.cnf_optim_num_slabs(n, offs, T))
        self._dev = {
            'device': device, 'n': n, 'T': T, 'num_slabs': num_slabs,
            'table': torch.from_numpy(host).to(device),
            'state': torch.zeros(2, device=device, dtype=torch.int64),
            'stats': torch.zeros(_lib.OPTIM_STATS_FLOATS, device=device, dtype=torch.float32),
            'scales': torch.ones(T, device=device, dtype=torch.float32),
            'ws': torch.empty(int(lib.cnf_optim_workspace_bytes(n, T, num_slabs)), device=device, dtype=torch.uint8),
        }
        return self._dev

    def _slots(self, params: torch.Tensor):
        if self._m is None or self._m.numel() != params.numel() or self._m.device != params.device:
            self._m = torch.zeros_like(params)
            self._v = torch.zeros_like(params)
            self._ema = params.detach().clone() if self.use_ema else None
        return self._m, self._v

    def apply_flat(self, params: torch.Tensor, grads: torch.Tensor):
        """One Adam step on the flat parameter vector (in place)."""
        m, v = self._slots(params)
        if self.guarded:
            st = self._device_state(params.device)
            if st['n'] != params.numel():
                raise ValueError(f'the bound tensor table covers {st["n"]} parameters, the vector has {params.numel()}')
            d = _lib.cnf_optim_desc(self.learning_rate, self.beta_1, self.beta_2, self.epsilon, self.clipvalue,
                                    self.clipnorm, self.global_clipnorm, int(self.skip_nonfinite),
                                    self.ema_momentum if self.use_ema else 0.0)
            self.iterations += 1
            check(_lib.load().cnf_optim_step(ptr(params), ptr(grads), ptr(m), ptr(v), ptr(self._ema), params.numel(),
                                             ptr(st['table']), st['num_slabs'], st['T'], C.byref(d), ptr(st['state']),
                                             ptr(st['stats']), ptr(st['scales']), ptr(st['ws']),
                                             torch.cuda.current_stream().cuda_stream), 'cnf_optim_step')
            return
        self.iterations += 1
        check(_lib.load().cnf_adam_step(ptr(params), ptr(grads), ptr(m), ptr(v), params.numel(), self.learning_rate,
                                        self.beta_1, self.beta_2, self.epsilon, self.iterations,
                                        torch.cuda.current_stream().cuda_stream), 'cnf_adam_step')

    # -- the guarded step's record of its last call (device tensors: reading one is the caller's sync) --
    def stats(self):
        """{'grad_norm': the global norm of the raw gradient, 'clip_norm': the norm global_clipnorm compares (after
        clipvalue and clipnorm), 'nonfinite': NaN / inf elements of the gradient, 'skipped': 1 if the last step was
        skipped, 'alpha': its step size, 'global_scale': S, 'scales': [T] the factor applied to each tensor}, as
        views of device tensors the next step overwrites; no host read here."""
        if self._dev is None:
            raise RuntimeError('stats() belongs to the guarded step: no clipping / EMA / skip option is set, or the '
                               'optimizer has not been bound to a model yet')
        s = self._dev['stats']
        return {'grad_norm': s[0], 'clip_norm': s[1], 'nonfinite': s[2], 'skipped': s[3], 'alpha': s[4],
                'global_scale': s[5], 'scales': self._dev['scales']}

    @property
    def steps_applied(self) -> int:
        """steps that changed the parameters (reads the device counter; the plain step counts on the host)"""
        return int(self._dev['state'][0]) if self._dev is not None else self.iterations

    @property
    def steps_skipped(self) -> int:
        return int(self._dev['state'][1]) if self._dev is not None else 0

    @property
    def ema(self):
        """the flat EMA vector (None before the first step or without use_ema)"""
        return self._ema
