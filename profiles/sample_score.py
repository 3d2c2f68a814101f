"""What scoring the draws inside the sampling call costs (cnf_flow_sample_score), cfg2, B = 8, S = 64, chunk = 64.
Host time of a call ending in a device synchronise: the median of `--steps` calls (default 20) after `--warmup`
(default 3). Every figure comes from a fresh process; the sides are alternated `--rounds` times (default 3) and
every round's median is printed.

  plain            cFlow.sample(y, 64, chunk=64, return_samples=False): mean and std only
  score            the same call with truth=, hist=(64, lo, hi) and quantiles=(0.05, 0.5, 0.95): mean, std, rank,
                   abs_err, sq_err, hist, quantiles; also the per-kernel GPU time of one such call by launch
                   timing (cnf_plan_set_launch_timing), summed per kernel name
  --baseline-root  also `plain` on the package of DIR, a built checkout of the commit to compare with: the
                   launches are the same, so the two must agree within the run-to-run span

    python profiles/sample_score.py [--baseline-root DIR]                 # everything, one JSON line
    python profiles/sample_score.py --side score                          # one side, one process
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from profiles.inverse_logdet import SAMPLE, _flow, _timed  # noqa: E402

HIST = (64, -6.0, 6.0)
LEVELS = (0.05, 0.5, 0.95)


def _kernel_times(torch, flow, call, reps=5):
    """{kernel name: [launches per call, GPU ms per call]} by launch timing, the mean of `reps` calls"""
    from arl_conditional_normalizing_flows_amd import _lib
    lib = _lib.load()
    plan = flow._plan
    _lib.check(lib.cnf_plan_set_launch_timing(plan, 1), 'timing on')
    per = {}
    try:
        for _ in range(reps):
            call()
            torch.cuda.synchronize()
            name, ms = C.create_string_buffer(256), C.c_float()
            fl, by = C.c_double(), C.c_double()
            for i in range(lib.cnf_plan_num_recorded_launches(plan)):
                _lib.check(lib.cnf_plan_recorded_launch_info(plan, i, name, 256, C.byref(fl), C.byref(by)), 'info')
                _lib.check(lib.cnf_plan_launch_time_ms(plan, i, C.byref(ms)), 'launch time')
                e = per.setdefault(name.value.decode(), [0, 0.0, 0.0])
                e[0] += 1
                e[1] += ms.value
                e[2] += by.value
    finally:
        _lib.check(lib.cnf_plan_set_launch_timing(plan, 0), 'timing off')
    return {k: [n // reps, t / reps, b / reps] for k, (n, t, b) in per.items()}


def run(side, steps, warmup):
    torch, flow, xy, cfg = _flow(SAMPLE['name'], SAMPLE['B'])
    y = xy[..., cfg.x_d:].contiguous()
    truth = xy[..., :cfg.x_d].contiguous()
    del xy
    kw = dict(seed=SAMPLE['seed'], chunk=SAMPLE['chunk'], return_samples=False)
    if side == 'score':
        kw.update(truth=truth, hist=HIST, quantiles=LEVELS)

    def call():
        return flow.sample(y, SAMPLE['S'], **kw)
    ms, peak = _timed(torch, call, steps, warmup)
    from arl_conditional_normalizing_flows_amd import _lib
    out = {'side': side, 'call_ms': ms, 'peak_bytes': peak, 'library': str(_lib.LIB_PATH)}
    if side == 'score':
        per = _kernel_times(torch, flow, call)
        total = sum(t for _, t, _ in per.values())
        out['gpu_ms_per_call'] = total
        out['kernels'] = {k: {'launches': n, 'ms': round(t, 5), 'bytes': b} for k, (n, t, b) in per.items()
                          if k.startswith(('k_sample', 'k_latent'))}
        out['inverse_ms'] = total - sum(t for k, (_, t, _) in per.items() if k.startswith(('k_sample', 'k_latent')))
        r = call()
        out['hist_total'] = int(r['hist'].sum())
    return out


def _child(argv):
    r = subprocess.run([sys.executable] + argv, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.exit(f'{argv} failed ({r.returncode}):\n{r.stdout}\n{r.stderr}')
    print(f'# done: {" ".join(argv[1:])}', file=sys.stderr, flush=True)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--side', choices=['plain', 'score'])
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--baseline-root', default=None)
    ap.add_argument('--root', default=None, help='with --side: import the package from this checkout')
    a = ap.parse_args()
    if a.side:
        if a.root:
            sys.path.insert(0, os.path.abspath(a.root))
        print(json.dumps(run(a.side, a.steps, a.warmup)))
        return
    me = os.path.abspath(__file__)
    res = {'baseline_plain': [], 'plain': [], 'score': []}
    for _ in range(a.rounds):
        for side in res:
            extra = []
            if side == 'baseline_plain':
                if not a.baseline_root:
                    continue
                extra = ['--root', a.baseline_root]
            res[side].append(_child([me, '--side', side.replace('baseline_', ''), '--steps', str(a.steps), '--warmup',
                                     str(a.warmup)] + extra))
    last = res['score'][-1]
    print(json.dumps({'sample': SAMPLE, 'hist': HIST, 'levels': LEVELS, 'steps': a.steps, 'warmup': a.warmup,
                      **{f'{k}_call_ms': [r['call_ms'] for r in v] for k, v in res.items()},
                      'libraries': sorted({r['library'] for v in res.values() for r in v}),
                      'score_gpu_ms_per_call': last['gpu_ms_per_call'], 'score_inverse_ms': last['inverse_ms'],
                      'score_kernels': last['kernels'], 'score_peak_bytes': last['peak_bytes'],
                      'plain_peak_bytes': res['plain'][-1]['peak_bytes'], 'hist_total': last['hist_total']}))


if __name__ == '__main__':
    main()
