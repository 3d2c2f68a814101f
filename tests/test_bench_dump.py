"""bench.py --dump-outputs: the writer behind it (CPU). float32 .npy per name, whole arrays while
they fit their share of the 64 MB budget, otherwise the same seeded sample on every call, so that
the dumps of two builds line up element for element."""
import os

import numpy as np
import torch

import bench


def test_dump_outputs_writes_float32_npy(tmp_path):
    a = torch.arange(24, dtype=torch.float64).reshape(2, 3, 4)
    b = np.arange(5, dtype=np.int64)
    bench.dump_outputs(str(tmp_path / 'd'), {'a': a, 'b': b})
    ra, rb = np.load(tmp_path / 'd' / 'a.npy'), np.load(tmp_path / 'd' / 'b.npy')
    assert ra.dtype == np.float32 and ra.shape == (2, 3, 4) and np.array_equal(ra, a.numpy())
    assert rb.dtype == np.float32 and np.array_equal(rb, b)
    bench.dump_outputs(str(tmp_path / 'd'), {'a': a}, rank=1)
    assert np.array_equal(np.load(tmp_path / 'd' / 'a_rank1.npy'), ra)


def test_dump_outputs_samples_within_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_BUDGET_BYTES', 4 * 200)     # 100 floats per array
    rng = np.random.default_rng(0)
    big, small = rng.standard_normal((30, 17)).astype(np.float32), rng.standard_normal(7).astype(np.float32)
    for d in ('one', 'two'):
        bench.dump_outputs(str(tmp_path / d), {'big': big, 'small': small})
    one, two = np.load(tmp_path / 'one' / 'big.npy'), np.load(tmp_path / 'two' / 'big.npy')
    assert one.shape == (100,) and np.array_equal(one, two)      # the same elements every time
    assert np.isin(one, big).all()
    assert np.array_equal(np.load(tmp_path / 'one' / 'small.npy'), small)
    total = sum(os.path.getsize(tmp_path / 'one' / f) for f in os.listdir(tmp_path / 'one'))
    assert total <= 4 * 200 + 2 * 128                            # data + the two .npy headers
