"""Host time of one posterior-sampling call of the toy flow, ending in a device synchronise, at the reference's
own configuration (TOYcINN.py:84-98: 24 coupling layers, H = 32, L = 6, x_d = 2), B = 8 conditions and
S = 125 000 draws each (10^6 draws):

  sample  cINN_affine.sample(y, S, return_samples=False, hist=(128, -4, 4)): mean / std and a 128 x 128
          histogram per condition from k_toy_sample + k_toy_sample_stats (no [B S, 3] tensor)
  loop    what a user writes without it, on the library's other kernels only: renew_noise
          (cnf_instance_noise) -> torch.cat with y -> call(zy, +1) (k_toy) -> torch.mean / torch.std over
          the draws; no histogram (torch.histogramdd has no device implementation)

Each side runs in a fresh process; the two are alternated `--rounds` times (default 3); a figure is the median
of `--steps` timed calls (default 20) after `--warmup` (default 3). Prints one JSON line: the per-round medians
of both sides, each side's peak device memory above the process's floor (the weights and y), the largest
difference between the two sides' means and stds, and for the sample side the device-event time of a
statistics-only call (k_toy_sample and the one-wave-per-element k_toy_sample_stats between two events).

    python profiles/toy_sample.py                 # the alternated comparison
    python profiles/toy_sample.py --side sample   # one side, one process
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KW = dict(io_shape=3, x_d=2, num_coupling_layers=24, intermediate_dims=32, num_layers=6)
B, S = 8, 125000
HIST = (128, -4.0, 4.0)
SEED = 3


def _setup():
    import torch
    from arl_conditional_normalizing_flows_amd.toy_model import cINN_affine
    dev = torch.device('cuda', 0)
    model = cINN_affine(**KW, device=dev, seed=0)
    y = torch.linspace(-1.0, 1.0, B, device=dev).reshape(B, 1).contiguous()
    return torch, model, y


def _timed(torch, call, steps, warmup):
    """(median host ms of a call ending in a synchronise, peak device bytes above the floor before the first call)"""
    torch.cuda.synchronize()
    floor = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), torch.cuda.max_memory_allocated() - floor


def run_sample(steps, warmup):
    torch, model, y = _setup()

    def call():
        return model.sample(y, S, seed=SEED, return_samples=False, hist=HIST)
    ms, peak = _timed(torch, call, steps, warmup)
    out = call()
    ev = []
    for i in range(warmup + steps):   # statistics only: k_toy_sample + k_toy_sample_stats
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        model.sample(y, S, seed=SEED, return_samples=False)
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ev.append(a.elapsed_time(b))
    return {'side': 'sample', 'call_ms': ms, 'peak_bytes': peak, 'kernel_ms': statistics.median(ev),
            'mean': out['mean'].cpu().tolist(), 'std': out['std'].cpu().tolist(),
            'inside': float(out['hist'].sum()) / (B * S)}


def run_loop(steps, warmup):
    torch, model, y = _setup()
    from arl_conditional_normalizing_flows_amd.base_functions import renew_noise
    x_d = model.x_d

    def call():
        z = renew_noise(torch.empty((B, S, x_d), device=y.device), seed=SEED, offset=0)
        zy = torch.cat([z, y[:, None].expand(B, S, 3 - x_d)], dim=-1).reshape(B * S, 3)
        xy, _ = model.call(zy, 1)
        x = xy[:, :x_d].reshape(B, S, x_d)
        return torch.mean(x, dim=1), torch.std(x, dim=1, unbiased=False)
    ms, peak = _timed(torch, call, steps, warmup)
    mean, std = call()
    return {'side': 'loop', 'call_ms': ms, 'peak_bytes': peak, 'mean': mean.cpu().tolist(), 'std': std.cpu().tolist()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--side', choices=['sample', 'loop'])
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    a = ap.parse_args()
    if a.side:
        print(json.dumps((run_sample if a.side == 'sample' else run_loop)(a.steps, a.warmup)))
        return
    res = {'sample': [], 'loop': []}
    for _ in range(a.rounds):
        for side in ('sample', 'loop'):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--side', side, '--steps', str(a.steps),
                                '--warmup', str(a.warmup)], capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit(f'{side} run failed ({r.returncode}):\n{r.stdout}\n{r.stderr}')
            res[side].append(json.loads(r.stdout.strip().splitlines()[-1]))
    s, l = res['sample'][-1], res['loop'][-1]

    def diff(k):
        return max(abs(p - q) for rs, rl in zip(s[k], l[k]) for p, q in zip(rs, rl))
    print(json.dumps({'config': KW, 'B': B, 'S': S, 'steps': a.steps, 'warmup': a.warmup,
                      'sample_call_ms': [r['call_ms'] for r in res['sample']],
                      'loop_call_ms': [r['call_ms'] for r in res['loop']],
                      'sample_kernel_ms': [r['kernel_ms'] for r in res['sample']],
                      'sample_peak_bytes': s['peak_bytes'], 'loop_peak_bytes': l['peak_bytes'],
                      'max_mean_diff': diff('mean'), 'max_std_diff': diff('std'), 'hist_inside': s['inside']}))


if __name__ == '__main__':
    main()
