"""What the fused batch assembly saves: one epoch of training batches at cfg2's shape (batch 64, 32x32x3 images,
'SR2,1', the 2 % baseline noise and an annealing noise stage), once through SuperResolutionDataset.with_noise (one
cnf_batch_assemble launch per batch) and once through the composed calls it replaces (per batch: a torch index
gather, preprocess_dataset_SR, instance_noise twice = 4 launches and 3 intermediate tensors). Both sides build the
epoch's order on the host and upload it once; the batches are dropped as they are made.

Device time between two events around one epoch of `--batches` batches (default 100), per batch; the median of
`--steps` epochs (default 20) after `--warmup` (default 3); the sides alternated `--rounds` times (default 3), every
round's median printed. Before timing, one epoch of both sides is compared bit for bit (`equal`).

    python profiles/batch_assemble.py               # one JSON line
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B, H, C = 64, 32, 3
SEED, SEED1, ALPHA1 = 0, 12345, 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, default=100)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch
    from arl_conditional_normalizing_flows_amd.base_functions import instance_noise, preprocess_dataset_SR
    from arl_conditional_normalizing_flows_amd.datasets import SuperResolutionDataset
    assert torch.cuda.is_available(), 'batch_assemble.py times the GPU: no device found'
    dev = torch.device('cuda', 0)
    n = a.batches * B
    imgs = torch.rand((n, H, H, C), generator=torch.Generator().manual_seed(0))
    ds = SuperResolutionDataset(imgs, B, 'SR2,1', seed=SEED, shuffle=False, renew_noise=False, device=dev)
    view = ds.with_noise(ALPHA1, SEED1)
    cache = ds.images
    per_batch = B * H * H * 2 * C

    def fused(keep=False):
        out = []
        for xy in view():
            if keep:
                out.append(xy)
        return out

    def composed(keep=False):
        order = np.random.Generator(np.random.Philox(key=[SEED, 0])).permutation(n).astype(np.int64)
        index = torch.from_numpy(order).to(dev)
        out = []
        for k in range(a.batches):
            xy = preprocess_dataset_SR(cache[index[k * B:(k + 1) * B]], 'SR2,1', True)
            xy = instance_noise(xy, 0.98, seed=SEED, offset=k * per_batch)
            xy = instance_noise(xy, ALPHA1, seed=SEED1, offset=k * per_batch)
            if keep:
                out.append(xy)
        return out

    equal = all(torch.equal(u, v) for u, v in zip(fused(True), composed(True)))

    def epoch_ms(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / a.batches

    sides = {'fused': fused, 'composed': composed}
    res = {k: [] for k in sides}
    for _ in range(a.rounds):
        for k, fn in sides.items():
            for _ in range(a.warmup):
                epoch_ms(fn)
            res[k].append(round(statistics.median(epoch_ms(fn) for _ in range(a.steps)), 5))
    med = {k: statistics.median(r) for k, r in res.items()}
    print(json.dumps({'batch': B, 'image': [H, H, C], 'batches_per_epoch': a.batches, 'steps': a.steps,
                      'warmup': a.warmup, 'equal': equal, 'launches_per_batch': {'fused': 1, 'composed': 4},
                      **{f'{k}_ms_per_batch': r for k, r in res.items()},
                      'fused_over_composed': round(med['fused'] / med['composed'], 4)}))


if __name__ == '__main__':
    main()
