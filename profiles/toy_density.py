"""Host time of one density heat map of the toy flow, ending in a device synchronise, at the reference's own
configuration (TOYcINN.py:84-98: 24 coupling layers, H = 32, L = 6, x_d = 2), B = 8 conditions and a grid of
G = 256 bins per component over [-4, 4) (65 536 points per condition, 524 288 in all):

  density  cINN_affine.density(y, 256, -4, 4): log_prob [B, G, G] and log_mass [B] from k_toy_density +
           k_toy_density_mass (no [B G^2, 3] tensor, no zy)
  loop     what a user writes without it, on the library's other kernels only: torch builds the [B G^2, 3] points
           (the same fp32 centres) -> call(xy, -1) (k_toy) -> the Gaussian term in torch -> torch.logsumexp

Each side runs in a fresh process; the two are alternated `--rounds` times (default 3); a figure is the median
of `--steps` timed calls (default 20) after `--warmup` (default 3). Prints one JSON line: the per-round medians
of both sides, each side's peak device memory above the process's floor (the weights and y), the largest
difference between the two sides' log_prob and log_mass, and for the density side the device-event time of a call
(the two kernels between two events).

    python profiles/toy_density.py                  # the alternated comparison
    python profiles/toy_density.py --side density   # one side, one process
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KW = dict(io_shape=3, x_d=2, num_coupling_layers=24, intermediate_dims=32, num_layers=6)
B, G = 8, 256
LO, HI = -4.0, 4.0


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


def _dump(path, torch, log_prob, log_mass):
    if path:
        torch.save({'log_prob': log_prob.reshape(B, -1).cpu(), 'log_mass': log_mass.cpu()}, path)


def run_density(steps, warmup, dump):
    torch, model, y = _setup()

    def call():
        return model.density(y, G, LO, HI)
    ms, peak = _timed(torch, call, steps, warmup)
    out = call()
    ev = []
    for i in range(warmup + steps):   # k_toy_density + k_toy_density_mass
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        model.density(y, G, LO, HI)
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ev.append(a.elapsed_time(b))
    _dump(dump, torch, out['log_prob'], out['log_mass'])
    return {'side': 'density', 'call_ms': ms, 'peak_bytes': peak, 'kernel_ms': statistics.median(ev),
            'log_mass': out['log_mass'].cpu().tolist()}


def run_loop(steps, warmup, dump):
    torch, model, y = _setup()
    x_d = model.x_d
    step = (torch.tensor(HI, dtype=torch.float32) - torch.tensor(LO, dtype=torch.float32)) / G   # fp32, as the kernel's
    log_cell = x_d * math.log(float(step))

    def call():
        c = LO + (torch.arange(G, device=y.device, dtype=torch.float32) + 0.5) * step.to(y.device)
        g0, g1 = torch.meshgrid(c, c, indexing='ij')
        pts = torch.stack([g0, g1], dim=-1).reshape(1, G * G, x_d).expand(B, -1, -1)
        xy = torch.cat([pts, y[:, None].expand(B, G * G, 3 - x_d)], dim=-1).reshape(B * G * G, 3)
        zy, ld = model.call(xy, -1)
        z = zy[:, :x_d]
        lp = (-0.5 * x_d * math.log(2.0 * math.pi) - 0.5 * (z * z).sum(-1) + ld).reshape(B, G * G)
        return lp, torch.logsumexp(lp, dim=1) + log_cell
    ms, peak = _timed(torch, call, steps, warmup)
    lp, lm = call()
    _dump(dump, torch, lp, lm)
    return {'side': 'loop', 'call_ms': ms, 'peak_bytes': peak, 'log_mass': lm.cpu().tolist()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--side', choices=['density', 'loop'])
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--dump', default='', help='write this side\'s log_prob / log_mass to a file (torch.save)')
    a = ap.parse_args()
    if a.side:
        print(json.dumps((run_density if a.side == 'density' else run_loop)(a.steps, a.warmup, a.dump)))
        return
    res = {'density': [], 'loop': []}
    with tempfile.TemporaryDirectory() as tmp:
        for _ in range(a.rounds):
            for side in ('density', 'loop'):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), '--side', side, '--steps', str(a.steps),
                                    '--warmup', str(a.warmup), '--dump', os.path.join(tmp, side + '.pt')],
                                   capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    sys.exit(f'{side} run failed ({r.returncode}):\n{r.stdout}\n{r.stderr}')
                res[side].append(json.loads(r.stdout.strip().splitlines()[-1]))
        import torch
        d, l = (torch.load(os.path.join(tmp, side + '.pt')) for side in ('density', 'loop'))
    diff = {k: float((d[k].double() - l[k].double()).abs().max()) for k in ('log_prob', 'log_mass')}
    print(json.dumps({'config': KW, 'B': B, 'G': G, 'lo': LO, 'hi': HI, 'steps': a.steps, 'warmup': a.warmup,
                      'density_call_ms': [r['call_ms'] for r in res['density']],
                      'loop_call_ms': [r['call_ms'] for r in res['loop']],
                      'density_kernel_ms': [r['kernel_ms'] for r in res['density']],
                      'density_peak_bytes': res['density'][-1]['peak_bytes'], 'loop_peak_bytes': res['loop'][-1]['peak_bytes'],
                      'max_log_prob_diff': diff['log_prob'], 'max_log_mass_diff': diff['log_mass'],
                      'log_prob_min': float(d['log_prob'].min()), 'log_prob_max': float(d['log_prob'].max()),
                      'log_mass': res['density'][-1]['log_mass']}))


if __name__ == '__main__':
    main()
