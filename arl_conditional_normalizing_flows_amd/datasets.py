"""Device-resident image datasets for `training.fit` / `anneal_and_fit` / `cFlow.train_step`: the data
half of the reference's driver (conv_cINN.py:209-508) as two callable datasets with the toy datasets'
protocol (`toy_datasets.py`): `ds()` returns the epoch's batches, `len(ds)` their number.

  ClassConditionalDataset   :209-331  one image array per class; preprocess_dataset_class, the label
                                      plane concatenated, each class cut to whole batches so that no
                                      batch mixes classes, the BATCH order shuffled per epoch (:328)
  SuperResolutionDataset    :400-508  one image array; preprocess_dataset_SR; EXAMPLES shuffled per
                                      epoch, then batched, the last batch possibly short (:450-454)

The images are uploaded once (fp32, NHWC) and stay on the device. Per epoch the order is built on the
host with numpy.random.Generator(numpy.random.Philox(key=[seed, epoch])), the epoch's index list (and
labels) go up in one copy each, and every batch is ONE launch of cnf_batch_assemble (cnf_transforms.hip)
on the current stream: gather, transform, label plane, the 2 % baseline noise the reference adds afresh
on every pass (instance_noise(., 0.98), :309-315, :437-442) and, on a `with_noise` view, the annealing
noise of `anneal_and_fit`. Batches are made lazily, one at a time.

Rules (DESIGN.md has them in full):
  noise stage 0   seed `seed`; the offset of a batch is the number of output elements of all batches
                  before it, in the GLOBAL (unsharded) batch list, carried on across epochs;
                  renew_noise=False restarts it every epoch (the reference's cached validation set)
  shuffle=False   every epoch has epoch 0's order
  shard=(r, w)    every rank builds the same global list and takes batches r, r + w, ... of it,
                  len(global) // w of them
  with_noise      a view of the same cache (and the same epoch / offset state) whose batches carry
                  noise stage 1; its offset advances per batch within a call and restarts on every call

device='cpu' runs the same plan over torch expressions on the host. That path is for tests of the
ordering logic; it is not a fallback (its values agree with the kernel's to rounding, not bit for bit).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .base_functions import _SR_TYPES

_M64 = 2 ** 64 - 1


# ---------------------------------------------------------------------------------------------
# the host path (tests): cnf_device.h's expressions in numpy / torch
# ---------------------------------------------------------------------------------------------
def _philox_normals(seed, g):
    """instance_noise_value's z of stream elements g (uint64 array): Philox4x32-10 + Box-Muller."""
    g = np.asarray(g, dtype=np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    c = [(g >> np.uint64(2)) & m32, (g >> np.uint64(34)) & m32, np.zeros_like(g), np.zeros_like(g)]
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1),
             p0 & m32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    w = (g & np.uint64(3)).astype(np.int64)
    a = np.where(w < 2, c[0], c[2])
    b = np.where(w < 2, c[1], c[3])
    u1 = ((a >> np.uint64(8)).astype(np.float32) + np.float32(1)) * np.float32(1.0 / 16777216.0)
    u2 = (b >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    rad = np.sqrt(np.float32(-2) * np.log(u1))
    th = np.float32(6.283185307179586) * u2
    return np.where(w & 1, rad * np.sin(th), rad * np.cos(th)).astype(np.float32)


def _noise_cpu(x, alpha, seed, offset):
    g = (np.arange(x.numel(), dtype=np.uint64) + np.uint64(offset & _M64))
    z = torch.from_numpy(_philox_normals(seed, g)).reshape(x.shape)
    return np.float32(alpha) * x + np.float32(1.0 - np.float32(alpha)) * z


def _logit_cpu(x, a):
    b = (1.0 - 2.0 * a) / (1.0 - a)
    lo, hi = np.log(np.float32(a / (1.0 - a))), np.log(np.float32((1.0 - a) / a))
    e = np.float32((1.0 - a) * b) * x + np.float32(a)
    return (torch.log(e / (1.0 - e)) - float(lo)) / float(hi - lo)


def _down_cpu(x):
    B, H, W, Cc = x.shape
    v = x.reshape(B, H // 2, 2, W // 2, 2, Cc)
    return ((v[:, :, 0, :, 0] + v[:, :, 0, :, 1]) + (v[:, :, 1, :, 0] + v[:, :, 1, :, 1])) * 0.25


def _sr_cpu(h, xd, yl, residual):
    for _ in range(xd):
        h = _down_cpu(h)
    y = h
    for _ in range(yl):
        y = _down_cpu(y)
    for _ in range(yl):
        y = y.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    return torch.cat([h - y if residual else h, y], dim=-1)


# ---------------------------------------------------------------------------------------------
# the datasets
# ---------------------------------------------------------------------------------------------
def _as_images(a, what):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
    if t.dim() != 4 or min(t.shape) < 1:
        raise ValueError(f'{what} must be a non-empty [n, H, W, C] array or tensor')
    return t


class _Epoch:
    """One epoch's batches of one rank: sized, and iterated lazily (one launch per batch)."""

    def __init__(self, ds, batches, index, labels):
        self._ds, self._batches, self._index, self._labels = ds, batches, index, labels

    def __len__(self):
        return len(self._batches)

    def __iter__(self):
        off1 = self._ds._offset1
        for lo, hi, off0 in self._batches:
            xy = self._ds._assemble(self._index[lo:hi], None if self._labels is None else self._labels[lo:hi],
                                    off0, off1)
            off1 += xy.numel()
            yield xy


class _ImageDataset:
    _mode = None

    def _init_common(self, images, batch_size, base_alpha, seed, shuffle, renew_noise, shard, device):
        self.batch_size = int(batch_size)
        if self.batch_size < 1:
            raise ValueError('batch_size must be >= 1')
        self.base_alpha = float(base_alpha)
        if not (0.0 <= self.base_alpha <= 1.0):
            raise ValueError('base_alpha must lie in [0, 1]')
        self.seed = int(seed)
        if not (0 <= self.seed <= _M64):
            raise ValueError('seed must be a non-negative 64-bit integer')
        self.shuffle, self.renew_noise = bool(shuffle), bool(renew_noise)
        if shard is None:
            shard = (0, 1)
        self.rank, self.world = int(shard[0]), int(shard[1])
        if self.world < 1 or not (0 <= self.rank < self.world):
            raise ValueError('shard must be (rank, world) with 0 <= rank < world')
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        # the cache: one upload, fp32, contiguous
        self.images = images.to(device=self.device, dtype=torch.float32).contiguous()
        self._alpha1, self._seed1, self._offset1 = 1.0, 0, 0
        self._state = {'epoch': 0, 'offset': 0}   # shared with the with_noise views
        n = len(self._global_batches(0))
        if n // self.world < 1:
            raise ValueError(f'{n} batches per epoch cannot be split over {self.world} ranks')
        self._len = n // self.world

    def __len__(self):
        return self._len

    def with_noise(self, alpha, seed, offset=0):
        """A view of the same cache (sharing the epoch and stage-0 offset state) whose batches carry noise
        stage 1: instance_noise(batch, alpha, seed, offset + elements of the call's earlier batches)."""
        alpha = float(alpha)
        if not (0.0 <= alpha <= 1.0):
            raise ValueError('alpha must lie in [0, 1]')
        v = object.__new__(type(self))
        v.__dict__.update(self.__dict__)
        v._alpha1, v._seed1, v._offset1 = alpha, int(seed) & _M64, int(offset)
        return v

    def _rng(self, epoch):
        return np.random.Generator(np.random.Philox(key=[self.seed, epoch if self.shuffle else 0]))

    def __call__(self):
        st = self._state
        epoch, base = st['epoch'], (st['offset'] if self.renew_noise else 0)
        glob = self._global_batches(epoch)
        offs = np.concatenate([[0], np.cumsum([len(ix) * self._elems_per_image for ix, _ in glob])])
        st['epoch'] = epoch + 1
        st['offset'] = base + int(offs[-1])
        mine = list(range(self.rank, len(glob), self.world))[:self._len]
        bounds = np.concatenate([[0], np.cumsum([len(glob[g][0]) for g in mine])])
        batches = [(int(bounds[k]), int(bounds[k + 1]), base + int(offs[g])) for k, g in enumerate(mine)]
        index = torch.from_numpy(np.concatenate([glob[g][0] for g in mine]).astype(np.int64)).to(self.device)
        labels = None
        if self._mode == _lib.BATCH_CLASS:
            lab = np.concatenate([np.full(len(glob[g][0]), glob[g][1], np.float32) for g in mine])
            labels = torch.from_numpy(lab).to(self.device)
        return _Epoch(self, batches, index, labels)

    def _assemble(self, index, labels, off0, off1):
        if self.device.type == 'cpu':
            return self._assemble_cpu(index, labels, off0, off1)
        b = int(index.numel())
        xy = torch.empty((b,) + self._out_shape, device=self.device, dtype=torch.float32)
        d = self._desc()
        d.alpha0, d.seed0, d.offset0 = self.base_alpha, self.seed, off0 & _M64
        d.alpha1, d.seed1, d.offset1 = self._alpha1, self._seed1, off1 & _M64
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream().cuda_stream
            _lib.check(_lib.load().cnf_batch_assemble(self.images.data_ptr(), self.images.shape[0], index.data_ptr(),
                                                      None if labels is None else labels.data_ptr(), C.byref(d),
                                                      xy.data_ptr(), b, stream), 'cnf_batch_assemble')
        return xy

    def _assemble_cpu(self, index, labels, off0, off1):
        v = self._transform_cpu(self.images[index], labels)
        if self.base_alpha != 1.0:
            v = _noise_cpu(v, self.base_alpha, self.seed, off0)
        if self._alpha1 != 1.0:
            v = _noise_cpu(v, self._alpha1, self._seed1, off1)
        return v.float().contiguous()


class ClassConditionalDataset(_ImageDataset):
    """The class-conditional pipeline (conv_cINN.py:209-331). images_per_class: one [n_k, H, W, C] array or
    tensor per class, values in [0, 1]. labels: one float per class, default k / (K - 1) (:220-228; a single
    class gets 0). Each class is cut to whole batches of batch_size (its last n_k % batch_size images are
    dropped, :270-277), batches hold consecutive images of one class, and the batch order is shuffled per
    epoch. logits / a: preprocess_dataset_class(LOGITS, a). Batches are [batch_size, H, W, C + 1]."""
    _mode = _lib.BATCH_CLASS

    def __init__(self, images_per_class, batch_size, labels=None, logits=False, a=0.01, base_alpha=0.98, seed=0,
                 shuffle=True, renew_noise=True, shard=None, device=None):
        cls = [_as_images(x, 'every entry of images_per_class') for x in images_per_class]
        if not cls:
            raise ValueError('images_per_class is empty')
        if any(x.shape[1:] != cls[0].shape[1:] for x in cls):
            raise ValueError('every class must have the same H, W, C')
        K = len(cls)
        if labels is None:
            labels = [k / (K - 1) if K > 1 else 0.0 for k in range(K)]
        self.labels = [float(v) for v in labels]
        if len(self.labels) != K:
            raise ValueError('labels must have one entry per class')
        self.logit_a = 0.0
        if logits:
            self.logit_a = float(a)
            if not (0.0 < self.logit_a < 0.5):
                raise ValueError('a must lie in (0, 0.5)')
        bs = int(batch_size)
        if bs >= 1 and any(x.shape[0] < bs for x in cls):
            raise ValueError('every class needs at least batch_size images')
        starts = np.concatenate([[0], np.cumsum([x.shape[0] for x in cls])])
        self._class_batches = [(np.arange(starts[k] + j * bs, starts[k] + (j + 1) * bs, dtype=np.int64), self.labels[k])
                               for k in range(K) if bs >= 1 for j in range(cls[k].shape[0] // bs)]
        _, H, W, Cc = cls[0].shape
        self._out_shape = (H, W, Cc + 1)
        self._elems_per_image = H * W * (Cc + 1)
        self._init_common(torch.cat([x.float() for x in cls]), batch_size, base_alpha, seed, shuffle, renew_noise,
                          shard, device)

    @classmethod
    def from_tfrecords(cls, paths, batch_size, **kw):
        """One TFRecord file per class (tfrecords.load_tfrecord)."""
        from .tfrecords import load_tfrecord
        return cls([load_tfrecord(p)[0] for p in paths], batch_size, **kw)

    def _global_batches(self, epoch):
        order = self._rng(epoch).permutation(len(self._class_batches))
        return [self._class_batches[i] for i in order]

    def _desc(self):
        H, W, D = self._out_shape
        return _lib.cnf_batch_desc(H=H, W=W, C=D - 1, mode=self._mode, logit_a=self.logit_a)

    def _transform_cpu(self, x, labels):
        if self.logit_a:
            x = _logit_cpu(x, self.logit_a)
        return torch.cat([x, labels[:, None, None, None].expand(x.shape[:3] + (1,))], dim=-1)


class SuperResolutionDataset(_ImageDataset):
    """The super-resolution pipeline (conv_cINN.py:400-508). images: [N, H, W, C] in [0, 1]. model_type /
    residual / y_levels as base_functions.preprocess_dataset_SR. The examples are shuffled per epoch, then
    batched; the last batch may be short. Batches are [b, H >> x_down, W >> x_down, 2 C]."""
    _mode = _lib.BATCH_SR

    def __init__(self, images, batch_size, model_type='SR2,1', residual=True, y_levels=None, base_alpha=0.98,
                 seed=0, shuffle=True, renew_noise=True, shard=None, device=None):
        x = _as_images(images, 'images')
        if model_type not in _SR_TYPES:
            raise ValueError(f'model_type must be one of {sorted(_SR_TYPES)}')
        self.x_down, self.y_levels = _SR_TYPES[model_type]
        if y_levels is not None:
            self.y_levels = int(y_levels)
        self.residual = bool(residual)
        N, H, W, Cc = x.shape
        lv = self.x_down + self.y_levels
        if self.y_levels < 0 or lv > 8 or H % (1 << lv) or W % (1 << lv):
            raise ValueError('H and W must be divisible by 2^(x_down + y_levels), y_levels >= 0, at most 8 levels')
        self._n = N
        self._out_shape = (H >> self.x_down, W >> self.x_down, 2 * Cc)
        self._elems_per_image = int(np.prod(self._out_shape))
        self._init_common(x, batch_size, base_alpha, seed, shuffle, renew_noise, shard, device)

    @classmethod
    def from_tfrecords(cls, path, batch_size, **kw):
        """One TFRecord file (tfrecords.load_tfrecord)."""
        from .tfrecords import load_tfrecord
        return cls(load_tfrecord(path)[0], batch_size, **kw)

    def _global_batches(self, epoch):
        order = self._rng(epoch).permutation(self._n).astype(np.int64)
        return [(order[i:i + self.batch_size], None) for i in range(0, self._n, self.batch_size)]

    def _desc(self):
        _, H, W, Cc = self.images.shape
        return _lib.cnf_batch_desc(H=H, W=W, C=Cc, mode=self._mode, logit_a=0.0, x_down=self.x_down,
                                   y_levels=self.y_levels, residual=int(self.residual))

    def _transform_cpu(self, x, labels):
        return _sr_cpu(x, self.x_down, self.y_levels, self.residual)
