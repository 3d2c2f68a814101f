"""What the input gradient costs next to the training step's forward + backward, and what an ascent step costs
(cnf_flow_score, cnf_flow_ascend): cfg2, B = 64, chunk = 64, all in one process on one build. Host time of a call
ending in a device synchronise: the median of `--steps` calls (default 20) after `--warmup` (default 3); the sides
are alternated `--rounds` times (default 3) and every round's median is printed.

  score     cnf_flow_score (grad_x, grad_y, log_prob) through the C ABI on its own workspace
  train     cnf_flow_forward_train + cnf_flow_backward on the same xy = concat(x, y) and the train workspace
  forward   cnf_flow_forward_train alone (what both contain)
  ascend    cFlow.ascend: (time of steps = 11 - time of steps = 1) / 10, the cost of one more ascent step

    python profiles/flow_score.py                 # one JSON line
    python profiles/flow_score.py --once score    # one score call and nothing else (for a kernel trace:
                                                  # rocprofv3 --kernel-trace --stats -- python ... --once score)
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from profiles.inverse_logdet import _flow  # noqa: E402

CASE = dict(name='cfg2', B=64, chunk=64)


def _median_ms(torch, call, steps, warmup):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--once', choices=['score', 'train', 'ascend'])
    a = ap.parse_args()
    from arl_conditional_normalizing_flows_amd import _lib
    from arl_conditional_normalizing_flows_amd._lib import check, ptr
    torch, flow, xy, cfg = _flow(CASE['name'], CASE['B'])
    B, chunk = CASE['B'], CASE['chunk']
    lib = _lib.load()
    x, y = xy[..., :cfg.x_d].contiguous(), xy[..., cfg.x_d:].contiguous()
    st = torch.cuda.current_stream().cuda_stream
    desc = _lib.cnf_score_desc(chunk, 0.0, 0)
    ws_s = torch.empty(int(lib.cnf_plan_score_workspace_bytes(flow._plan, B, C.byref(desc))), device=xy.device,
                       dtype=torch.uint8)
    ws_t = torch.empty(int(lib.cnf_plan_train_workspace_bytes(flow._plan, B)), device=xy.device, dtype=torch.uint8)
    gx, gy, lp = torch.empty_like(x), torch.empty_like(y), torch.empty(B, device=xy.device)
    zy, ld, dp = torch.empty_like(xy), torch.empty(B, device=xy.device), torch.empty(flow.num_params, device=xy.device)

    def score():
        check(lib.cnf_flow_score(flow._plan, ptr(flow.params), ptr(flow._aux), ptr(x), ptr(y), C.byref(desc), ptr(gx),
                                 ptr(gy), ptr(lp), ptr(ws_s), B, st), 'cnf_flow_score')

    def forward():
        check(lib.cnf_flow_forward_train(flow._plan, ptr(flow.params), ptr(flow._aux), ptr(xy), ptr(zy), ptr(ld),
                                         ptr(ws_t), B, st), 'cnf_flow_forward_train')

    def train():
        forward()
        check(lib.cnf_flow_backward(flow._plan, ptr(flow.params), ptr(xy), ptr(zy), ptr(ws_t), B, 1.0 / B, ptr(dp), st),
              'cnf_flow_backward')

    def ascend(steps):
        return lambda: flow.ascend(x, y, steps, chunk=chunk)

    if a.once:
        {'score': score, 'train': train, 'ascend': ascend(1)}[a.once]()
        torch.cuda.synchronize()
        return
    sides = {'score': score, 'train': train, 'forward': forward, 'ascend_1': ascend(1), 'ascend_11': ascend(11)}
    res = {k: [] for k in sides}
    for _ in range(a.rounds):
        for k, fn in sides.items():
            res[k].append(round(_median_ms(torch, fn, a.steps, a.warmup), 4))
    out = {'case': CASE, 'steps': a.steps, 'warmup': a.warmup, **{f'{k}_ms': v for k, v in res.items()},
           'ascend_step_ms': [round((b - s) / 10.0, 4) for s, b in zip(res['ascend_1'], res['ascend_11'])],
           'score_over_train': [round(s / t, 4) for s, t in zip(res['score'], res['train'])]}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
