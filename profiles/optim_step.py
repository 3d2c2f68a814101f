"""What the guarded Adam step costs next to the plain one, on cfg2's flat parameter vector and tensor table
(n = cfg2's parameter count), all in one process on one build. Device time between two events around `--calls`
consecutive calls (default 50), divided by the calls; the median of `--steps` such windows (default 30) after
`--warmup` windows (default 3); the sides are alternated `--rounds` times (default 3), every round's median printed.

  adam       cnf_adam_step (k_adam), the reference
  clip       cnf_optim_step with clipnorm = 1 (k_optim_stats + k_optim_finish + k_optim_step)
  clip_ema   the same with ema_momentum = 0.99

Bytes per element: k_adam 7 words (reads p, g, m, v; writes p, m, v); clipping reads g once more (8); the EMA reads
and writes e (10).

    python profiles/optim_step.py                   # one JSON line
    python profiles/optim_step.py --once clip_ema   # `--calls` calls of one side and nothing else (for a kernel
                                                    # trace: rocprofv3 --kernel-trace --stats -- python ... --once clip_ema)
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LR, B1, B2, EPSILON = 3e-4, 0.9, 0.999, 1e-7


def _window_ms(torch, call, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def _median_ms(torch, call, calls, steps, warmup):
    for _ in range(warmup):
        _window_ms(torch, call, calls)
    return statistics.median(_window_ms(torch, call, calls) for _ in range(steps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--once', choices=['adam', 'clip', 'clip_ema'])
    a = ap.parse_args()
    import torch
    from arl_conditional_normalizing_flows_amd import _lib
    from arl_conditional_normalizing_flows_amd._lib import check, ptr
    from arl_conditional_normalizing_flows_amd.config import PRESETS
    from arl_conditional_normalizing_flows_amd.make_model import cFlow
    assert torch.cuda.is_available(), 'optim_step.py times the GPU: no device found'
    dev = torch.device('cuda', 0)
    lib = _lib.load()
    flow = cFlow(**PRESETS['cfg2'].kwargs(), device=dev)
    n = flow.num_params
    offsets = [o for _, o, _ in flow.param_specs] + [n]
    T = len(offsets) - 1
    del flow
    co = (C.c_int64 * (T + 1))(*offsets)
    import numpy as np
    host = np.zeros(int(lib.cnf_optim_table_bytes(n, co, T)), np.uint8)
    check(lib.cnf_optim_table_build(n, co, T, host.ctypes.data), 'cnf_optim_table_build')
    num_slabs = int(lib.cnf_optim_num_slabs(n, co, T))
    table = torch.from_numpy(host).to(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    p = torch.randn(n, device=dev, generator=gen) * 0.1
    g = torch.randn(n, device=dev, generator=gen) * 1e-3
    m, v, e = torch.zeros_like(p), torch.zeros_like(p), p.clone()
    state = torch.zeros(2, device=dev, dtype=torch.int64)
    stats = torch.zeros(_lib.OPTIM_STATS_FLOATS, device=dev)
    scales = torch.zeros(T, device=dev)
    ws = torch.empty(int(lib.cnf_optim_workspace_bytes(n, T, num_slabs)), device=dev, dtype=torch.uint8)
    st = torch.cuda.current_stream().cuda_stream
    step = [0]

    def adam():
        step[0] += 1
        check(lib.cnf_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), n, LR, B1, B2, EPSILON, step[0], st), 'cnf_adam_step')

    def optim(ema_momentum):
        d = _lib.cnf_optim_desc(LR, B1, B2, EPSILON, 0.0, 1.0, 0.0, 0, ema_momentum)

        def call():
            check(lib.cnf_optim_step(ptr(p), ptr(g), ptr(m), ptr(v), ptr(e), n, ptr(table), num_slabs, T, C.byref(d),
                                     ptr(state), ptr(stats), ptr(scales), ptr(ws), st), 'cnf_optim_step')
        return call

    sides = {'adam': adam, 'clip': optim(0.0), 'clip_ema': optim(0.99)}
    if a.once:
        for _ in range(a.calls):
            sides[a.once]()
        torch.cuda.synchronize()
        return
    res = {k: [] for k in sides}
    for _ in range(a.rounds):
        for k, fn in sides.items():
            res[k].append(round(_median_ms(torch, fn, a.calls, a.steps, a.warmup), 5))
    med = {k: statistics.median(r) for k, r in res.items()}
    out = {'n': n, 'tensors': T, 'slabs': num_slabs, 'calls': a.calls, 'steps': a.steps, 'warmup': a.warmup,
           **{f'{k}_ms': r for k, r in res.items()},
           'clip_over_adam': round(med['clip'] / med['adam'], 4), 'byte_ratio_clip': round(8 / 7, 4),
           'clip_ema_over_adam': round(med['clip_ema'] / med['adam'], 4), 'byte_ratio_clip_ema': round(10 / 7, 4),
           'adam_GBps': round(7 * 4 * n / med['adam'] / 1e6, 1), 'clip_GBps': round(8 * 4 * n / med['clip'] / 1e6, 1),
           'clip_ema_GBps': round(10 * 4 * n / med['clip_ema'] / 1e6, 1)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
