"""What cFlow.log_prob costs next to the forward it wraps, and what the by-hand recipe costs for the same pairs
(cnf_flow_log_prob): cfg2, B = 8 images x K = 10 conditions, chunk = 64, logit_a = 0.01.
Host time of a call ending in a device synchronise: the median of `--steps` calls (default 20) after `--warmup`
(default 3), each side in a fresh process, alternated `--rounds` times (default 3).

  log_prob   model.log_prob(x, y, pairwise=True, chunk=64, logit_a=0.01, return_posterior=True); also the GPU
             time of one such call by launch timing (cnf_plan_set_launch_timing), summed per kernel name, and
             the share of it spent in k_logp_gather, k_logp_finish and k_logp_posterior
  recipe     the same pairs without it (INTEGRATION.md's "before"): the [B*K,H,W,D] tensor by torch ops,
             preprocess_dataset_class(LOGITS=True) and its log-Jacobian by torch ops, the forward 64 images at a
             time, nll_sums, llz + logdet + log_jac, torch.log_softmax

    python profiles/flow_log_prob.py                   # everything, one JSON line
    python profiles/flow_log_prob.py --side log_prob   # one side, one process
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from profiles.inverse_logdet import _child, _flow, _timed  # noqa: E402
from profiles.sample_score import _kernel_times  # noqa: E402

CASE = dict(name='cfg2', B=8, K=10, chunk=64, logit_a=0.01)


def _inputs():
    from arl_conditional_normalizing_flows_amd.base_functions import de_logitify
    torch, flow, xy, cfg = _flow(CASE['name'], max(CASE['B'], CASE['K']))
    x = de_logitify(xy[:CASE['B'], ..., :cfg.x_d].contiguous(), CASE['logit_a'])
    y = xy[:CASE['K'], ..., cfg.x_d:].contiguous()
    return torch, flow, x, y, cfg


def run_log_prob(steps, warmup):
    torch, flow, x, y, cfg = _inputs()

    def call():
        return flow.log_prob(x, y, pairwise=True, chunk=CASE['chunk'], logit_a=CASE['logit_a'], return_posterior=True)
    ms, peak = _timed(torch, call, steps, warmup)
    per = _kernel_times(torch, flow, call)
    total = sum(t for _, t, _ in per.values())
    new = {k: {'launches': n, 'ms': round(t, 5), 'bytes': b} for k, (n, t, b) in per.items() if k.startswith('k_logp')}
    out = call()
    return {'side': 'log_prob', 'call_ms': ms, 'peak_bytes': peak, 'gpu_ms_per_call': total, 'kernels': new,
            'new_kernels_ms': sum(v['ms'] for v in new.values()),
            'new_kernels_share': sum(v['ms'] for v in new.values()) / total,
            'log_prob': out['log_prob'].cpu().tolist(), 'posterior_row0': out['posterior'][0].cpu().tolist()}


def run_recipe(steps, warmup):
    torch, flow, x, y, cfg = _inputs()
    from arl_conditional_normalizing_flows_amd.base_functions import preprocess_dataset_class
    B, K, a = CASE['B'], CASE['K'], CASE['logit_a']
    H, W, D = cfg.io_shape
    c1 = 1.0 - 2.0 * a
    span = math.log((1 - a) / a) - math.log(a / (1 - a))

    def call():
        e = a + c1 * x
        log_jac = (math.log(c1) - math.log(span) - torch.log(e) - torch.log1p(-e)).reshape(B, -1).sum(1)
        v = preprocess_dataset_class(x, LOGITS=True, a=a)
        xy = torch.cat([v[:, None].expand(B, K, H, W, cfg.x_d), y[None].expand(B, K, H, W, D - cfg.x_d)],
                       dim=-1).reshape(B * K, H, W, D).contiguous()
        lp = []
        for i in range(0, B * K, CASE['chunk']):
            part = xy[i:i + CASE['chunk']]
            zy, ld = flow(part, 1, per_image_logdet=True)
            _, per = flow.nll_sums(part, zy, ld)
            lp.append(per[:, 0] + per[:, 2])
        log_prob = torch.cat(lp).reshape(B, K) + log_jac[:, None]
        return log_prob, torch.log_softmax(log_prob.double(), dim=1).exp()
    ms, peak = _timed(torch, call, steps, warmup)
    return {'side': 'recipe', 'call_ms': ms, 'peak_bytes': peak, 'log_prob': call()[0].cpu().tolist()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--side', choices=['log_prob', 'recipe'])
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    a = ap.parse_args()
    if a.side:
        print(json.dumps({'log_prob': run_log_prob, 'recipe': run_recipe}[a.side](a.steps, a.warmup)))
        return
    me = os.path.abspath(__file__)
    res = {'log_prob': [], 'recipe': []}
    for _ in range(a.rounds):
        for side in res:
            res[side].append(_child([me, '--side', side, '--steps', str(a.steps), '--warmup', str(a.warmup)]))
    last, rec = res['log_prob'][-1], res['recipe'][-1]
    print(json.dumps({'case': CASE, 'steps': a.steps, 'warmup': a.warmup,
                      'log_prob_call_ms': [r['call_ms'] for r in res['log_prob']],
                      'recipe_call_ms': [r['call_ms'] for r in res['recipe']],
                      'gpu_ms_per_call': last['gpu_ms_per_call'], 'kernels': last['kernels'],
                      'new_kernels_ms': last['new_kernels_ms'],
                      'new_kernels_share': [r['new_kernels_share'] for r in res['log_prob']],
                      'log_prob_peak_bytes': last['peak_bytes'], 'recipe_peak_bytes': rec['peak_bytes'],
                      'max_log_prob_diff': max(abs(p - q) for rp, rq in zip(last['log_prob'], rec['log_prob'])
                                               for p, q in zip(rp, rq))}))


if __name__ == '__main__':
    main()
