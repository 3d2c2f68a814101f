"""Two-level super-resolution at inference, fused against by hand. Stage 1 is the reference's 'SR4,2' shape, 14x14x2
with squeeze_factor_block_list [0,0,0,0] (conv_cINN.py:55,171-175), stage 2 the preset 'ref_default', 28x28x2.
B = 8 degraded inputs, S = (16, 8): 128 high-resolution draws per input; per-pixel mean and std of the leaves plus
the truth scores (rank, abs_err, sq_err); no samples returned. Host time of a call ending in a device
synchronise: the median of `--steps` calls (default 20) after `--warmup` (default 3), and the peak device memory
above the process floor (flows and inputs allocated). Every figure comes from a fresh process; the sides are
alternated `--rounds` times (default 3) and every round's median is kept.

  cascade   cFlowCascade([f1, f2]).sample(y1, (16, 8), residual=True, return_samples=False, truth=truth)
  by_hand   f1.sample(y1, 16) -> reshape -> base_functions.up -> f2.sample(., 8) on the 128 conditions, then torch
            reductions over the [8, 128, 28, 28, 1] leaves: mean, std, (leaves < truth).sum, mean |leaves - truth|,
            sum (leaves - truth)^2. Only calls the parent commit has.

    python profiles/cascade_sample.py [--out profiles/cascade_sample.json]   # both sides, one JSON line
    python profiles/cascade_sample.py --side cascade                         # one side, one process
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from profiles.inverse_logdet import _timed  # noqa: E402

CASE = dict(B=8, S=(16, 8), seed=3, residual=True)
STAGE1 = dict(io_shape=(14, 14, 2), x_d=1, squeeze_factor_block_list=(0, 0, 0, 0), ResNeXt_block_list=(3, 3, 3, 3),
              num_kernels_list=(64, 64, 32, 32), cardinality_list=(8, 8, 4, 4))


def _setup():
    import numpy as np
    import torch
    from arl_conditional_normalizing_flows_amd.base_functions import up
    from arl_conditional_normalizing_flows_amd.config import PRESETS
    from arl_conditional_normalizing_flows_amd.make_model import cFlow
    dev = torch.device('cuda', 0)
    f1 = cFlow(**STAGE1, device=dev, seed=1)
    f2 = cFlow(**PRESETS['ref_default'].kwargs(), device=dev, seed=2)
    rng = np.random.default_rng(1)
    low = torch.from_numpy(rng.random((CASE['B'], 7, 7, 1), dtype=np.float32)).to(dev)
    y1 = up(low).contiguous()                       # the 4x4-degraded image, shown at 14x14
    truth = torch.from_numpy(rng.random((CASE['B'], 28, 28, 1), dtype=np.float32)).to(dev)
    return torch, up, f1, f2, y1, truth


def run(side, steps, warmup):
    torch, up, f1, f2, y1, truth = _setup()
    B, (S1, S2), seed, residual = CASE['B'], CASE['S'], CASE['seed'], CASE['residual']
    if side == 'cascade':
        from arl_conditional_normalizing_flows_amd.make_model import cFlowCascade
        cas = cFlowCascade([f1, f2])

        def call():
            return cas.sample(y1, (S1, S2), seed=seed, residual=residual, return_samples=False, truth=truth)
    else:
        off2 = B * S1 * 14 * 14

        def call():
            s1 = f1.sample(y1, S1, seed=seed, residual=residual, return_stats=False)['samples']
            cond = up(s1.reshape(B * S1, 14, 14, 1))
            s2 = f2.sample(cond, S2, seed=seed, offset=off2, residual=residual, return_stats=False)['samples']
            leaves = s2.reshape(B, S1 * S2, 28, 28, 1)
            t = truth[:, None]
            d = leaves - t
            return {'mean': leaves.mean(1), 'std': leaves.std(1, unbiased=False),
                    'rank': (leaves < t).sum(1, dtype=torch.int32), 'abs_err': d.abs().mean(1),
                    'sq_err': (d.double() ** 2).sum((2, 3, 4)).float()}
    ms, peak = _timed(torch, call, steps, warmup)
    r = call()
    torch.cuda.synchronize()
    return {'side': side, 'call_ms': ms, 'peak_bytes': peak, 'mean_of_mean': float(r['mean'].mean()),
            'rank_sum': int(r['rank'].sum())}


def _child(argv):
    r = subprocess.run([sys.executable] + argv, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.exit(f'{argv} failed ({r.returncode}):\n{r.stdout}\n{r.stderr}')
    print(f'# done: {" ".join(argv[1:])}', file=sys.stderr, flush=True)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--side', choices=['cascade', 'by_hand'])
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=None, help='also write the JSON result to this file')
    a = ap.parse_args()
    if a.side:
        print(json.dumps(run(a.side, a.steps, a.warmup)))
        return
    me = os.path.abspath(__file__)
    res = {'cascade': [], 'by_hand': []}
    for _ in range(a.rounds):
        for side in res:
            res[side].append(_child([me, '--side', side, '--steps', str(a.steps), '--warmup', str(a.warmup)]))
    out = {'case': CASE, 'stage1': STAGE1, 'stage2': 'ref_default', 'steps': a.steps, 'warmup': a.warmup,
           **{f'{k}_call_ms': [r['call_ms'] for r in v] for k, v in res.items()},
           **{f'{k}_peak_bytes': [r['peak_bytes'] for r in v] for k, v in res.items()},
           # the two sides draw the same leaves: the same rank total, the same mean up to the reduction order
           **{f'{k}_rank_sum': v[-1]['rank_sum'] for k, v in res.items()},
           **{f'{k}_mean_of_mean': v[-1]['mean_of_mean'] for k, v in res.items()}}
    line = json.dumps(out)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
