"""The crescents data of the toy driver (`TOYcINN_make_datasets.make_moons_dataset`, :17-270), as a
callable dataset for `training.fit` / `anneal_and_fit`.

Reference semantics kept: two crescents (class 0: (cos a, sin a); class 1: (1 - cos a,
1 - sin a - 0.5), or + 0.25 with label 2 when `overlapping`), angle ~ U(0, pi), N(0, noise) added to
both coordinates, every column standardised with the float32 mean / std of one 10^4-per-crescent
cloud on an even angle grid (:99-126), batched BEFORE shuffling so that a batch holds one class only
(:265-267), and new points every epoch (the tf.data pipeline re-draws on each iteration; here the
dataset is re-invoked per epoch by `training.fit`).

The sector datasets (`make_continuous_sectors`, `make_discrete_sectors`, :1114-1300) are the reference's data
with a continuous condition: y is an angle, x a point of the unit disc's sector around it. The mixed dataset
(`make_mixed_dataset`, its shape library) is out of scope.
"""
from __future__ import annotations

import math

import numpy as np
import torch


class make_moons_dataset:
    """Callable: each call returns an iterator over 2 * num_batches_per_class batches [batch_size, 3]
    (x0, x1, label; standardised, fp32) on `device`, single-class per batch, in shuffled batch
    order, with points drawn afresh. `device=None` is the current ROCm device; 'cpu' works too."""

    def __init__(self, num_batches_per_class, batch_size, noise=0.05, overlapping=False, seed=0, device=None):
        self.num_batches_per_class = int(num_batches_per_class)
        self.batch_size = int(batch_size)
        self.noise = float(noise)
        self.overlapping = bool(overlapping)
        if self.num_batches_per_class < 1 or self.batch_size < 1:
            raise ValueError('num_batches_per_class and batch_size must be >= 1')
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        self.shift = 0.25 if self.overlapping else -0.5
        self.label1 = 2.0 if self.overlapping else 1.0
        # the standardisation cloud (:111-126): an even angle grid, one noise draw, float32 statistics
        rng = np.random.default_rng(seed)
        t = np.linspace(0.0, math.pi, 10 ** 4)
        x = np.concatenate([np.cos(t), 1.0 - np.cos(t)])
        y = np.concatenate([np.sin(t), 1.0 - np.sin(t) + self.shift])
        cloud = np.stack([x, y], axis=1) + rng.normal(0.0, self.noise, (2 * 10 ** 4, 2))
        cloud = np.concatenate([cloud, np.repeat([0.0, self.label1], 10 ** 4)[:, None]], axis=1)
        self.mean = torch.from_numpy(cloud.mean(axis=0).astype(np.float32)).to(self.device)
        self.std = torch.from_numpy(cloud.std(axis=0).astype(np.float32)).to(self.device)
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(int(seed) + 1)
        self._order = torch.Generator()
        self._order.manual_seed(int(seed) + 2)

    def __len__(self):
        return 2 * self.num_batches_per_class

    def __call__(self):
        n, bs = self.num_batches_per_class, self.batch_size
        ang = torch.rand((2, n * bs), generator=self._gen, device=self.device) * math.pi
        eps = torch.randn((2, n * bs, 2), generator=self._gen, device=self.device) * self.noise
        c, s = torch.cos(ang), torch.sin(ang)
        x0 = torch.stack([c[0], 1.0 - c[1]])
        x1 = torch.stack([s[0], 1.0 - s[1] + self.shift])
        lab = torch.stack([torch.zeros_like(ang[0]), torch.full_like(ang[1], self.label1)])
        xy = torch.stack([x0 + eps[..., 0], x1 + eps[..., 1], lab], dim=-1)        # [2, n * bs, 3]
        xy = ((xy - self.mean) / self.std).reshape(2 * n, bs, 3)                   # batch, THEN shuffle
        order = torch.randperm(2 * n, generator=self._order).tolist()
        return iter([xy[i] for i in order])


def _sector_rows(rng, y, sector_width):
    """(r cos a, r sin a, y) per entry of y: a ~ U(y - width/2, y + width/2), r = sqrt(U(0, 1)), i.e. uniform
    over the sector of the unit disc (TOYcINN_make_datasets.py:1152-1175); float32, not standardised (:1177)."""
    ang = rng.uniform(y - sector_width / 2.0, y + sector_width / 2.0)
    r = np.sqrt(rng.uniform(0.0, 1.0, y.shape))
    return np.stack([r * np.cos(ang), r * np.sin(ang), y], axis=1).astype(np.float32)


class make_continuous_sectors:
    """`TOYcINN_make_datasets.make_continuous_sectors` (:1114-1205): each call returns the list of batches
    [batch_size, 3] (the last one shorter when batch_size does not divide num_points) of (x0, x1, y) on
    `device`: y ~ U[0, 2 pi) per point, x uniform over the sector of the unit disc centred on angle y with
    angular width sector_width. New points every call, from a numpy generator seeded once."""

    def __init__(self, num_points, batch_size, sector_width, seed=0, device=None):
        self.num_points, self.batch_size = int(num_points), int(batch_size)
        self.sector_width = float(sector_width)
        if self.num_points < 1 or self.batch_size < 1:
            raise ValueError('num_points and batch_size must be >= 1')
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        self._rng = np.random.default_rng(seed)

    def __len__(self):
        return (self.num_points + self.batch_size - 1) // self.batch_size

    def __call__(self):
        y = self._rng.uniform(0.0, 2.0 * math.pi, self.num_points)
        # (a float64 draw just below 2 pi may round up to float32(2 pi), which is above it: keep y in [0, 2 pi))
        y = np.minimum(y.astype(np.float32), np.nextafter(np.float32(2.0 * math.pi), np.float32(0.0))).astype(np.float64)
        xy = torch.from_numpy(_sector_rows(self._rng, y, self.sector_width)).to(self.device)
        return list(torch.split(xy, self.batch_size))


class make_discrete_sectors:
    """`TOYcINN_make_datasets.make_discrete_sectors` (:1207-1300): each call returns one batch
    [num_points_per_sector, 3] per entry of which_sectors, in their order, with y that entry (as float32)."""

    def __init__(self, num_points_per_sector, which_sectors, sector_width, seed=0, device=None):
        self.num_points_per_sector = int(num_points_per_sector)
        self.which_sectors = [float(np.float32(v)) for v in which_sectors]
        self.sector_width = float(sector_width)
        if self.num_points_per_sector < 1 or not self.which_sectors:
            raise ValueError('num_points_per_sector must be >= 1 and which_sectors non-empty')
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        self._rng = np.random.default_rng(seed)

    def __len__(self):
        return len(self.which_sectors)

    def __call__(self):
        y = np.repeat(np.asarray(self.which_sectors, np.float64), self.num_points_per_sector)
        xy = torch.from_numpy(_sector_rows(self._rng, y, self.sector_width)).to(self.device)
        return list(torch.split(xy, self.num_points_per_sector))
