"""Host time of one toy training step on the GPU, ending in a device synchronise, at the reference's
own configuration (TOYcINN.py:84-98: 24 coupling layers, H = 32, L = 6, x_d = 2) and B = 1000:

  hip    cINN_affine.train_step (k_toy + k_nll_sums + k_toy_bwd + k_toy_grad_sum + k_adam)
  torch  the loop a user could write on this stack without the library: the same model as torch fp32
         ops on the same GPU, autograd, torch.optim.Adam(eps=1e-7)

Each side runs in a fresh process; the two are alternated `--rounds` times (default 3); a figure is the
median of `--steps` timed steps (default 20) after `--warmup` (default 3). Prints one JSON line with
the per-round medians of both sides, and for the hip side the device-event time of cnf_toy_backward alone.

    python profiles/toy_train_step.py                 # the alternated comparison
    python profiles/toy_train_step.py --side hip      # one side, one process
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
B = 1000
LR = 1e-4   # TOYcINN.py:213-304


def _setup():
    import torch
    from arl_conditional_normalizing_flows_amd.toy_datasets import make_moons_dataset
    from arl_conditional_normalizing_flows_amd.toy_model import cINN_affine
    dev = torch.device('cuda', 0)
    model = cINN_affine(**KW, device=dev, seed=0)
    halves = list(make_moons_dataset(1, B // 2, seed=0, device=dev)())
    return torch, model, torch.cat(halves).contiguous()


def _timed(torch, step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def run_hip(steps, warmup):
    import ctypes as C
    torch, model, xy = _setup()
    from arl_conditional_normalizing_flows_amd import _lib
    from arl_conditional_normalizing_flows_amd.optimizers import Adam
    model.compile(optimizer=Adam(learning_rate=LR))
    out = {'side': 'hip', 'step_ms': _timed(torch, lambda: model.train_step(xy), steps, warmup)}
    # the backward (k_toy_bwd + k_toy_grad_sum) alone, by device events
    lib = _lib.load()
    ws, grads = model._train_workspace(B)
    zy = torch.empty_like(xy)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.cnf_toy_forward_train(C.byref(model._desc), model.params.data_ptr(), xy.data_ptr(), zy.data_ptr(),
                                         None, ws.data_ptr(), B, st), 'cnf_toy_forward_train')
    ev = []
    for i in range(warmup + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.check(lib.cnf_toy_backward(C.byref(model._desc), model.params.data_ptr(), xy.data_ptr(), zy.data_ptr(),
                                        ws.data_ptr(), B, 1.0 / B, grads.data_ptr(), st), 'cnf_toy_backward')
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ev.append(a.elapsed_time(b))
    out['backward_ms'] = statistics.median(ev)
    out['loss'] = float(model.log_loss(xy)[0])   # after warmup + steps updates, as the torch side reports
    return out


def run_torch(steps, warmup):
    torch, model, xy = _setup()
    from arl_conditional_normalizing_flows_amd.toy_model import MASK_U1
    lrelu = torch.nn.functional.leaky_relu
    flat = model.params.detach().clone()
    T, o = {}, 0
    for n, s in model.param_specs():
        size = s[0] * (s[1] if len(s) > 1 else 1)
        T[n] = flat[o:o + size].reshape(s).clone().requires_grad_(True)
        o += size
    opt = torch.optim.Adam(list(T.values()), lr=LR, eps=1e-7)
    L, x_d, lam = model.num_layers, model.x_d, float(model.lambda_y)

    def net(u1, j, blk):
        h = u1
        for k in range(L + 1):
            h = lrelu(h @ T[f't{j}.{blk}.d{k}.kernel'] + T[f't{j}.{blk}.d{k}.bias'], 0.3)
        return h @ T[f't{j}.{blk}.d{L + 1}.kernel'] + T[f't{j}.{blk}.d{L + 1}.bias']

    def forward():
        u = xy
        ld = torch.zeros(B, device=xy.device)
        for i in reversed(range(model.num_coupling_layers)):
            j = model.mask_indices[i]
            i1 = MASK_U1[j % 6]
            i2 = [c for c in range(3) if c not in i1]
            u1, u2 = u[:, i1], u[:, i2]
            A = torch.tanh(net(u1, j, 'A'))
            v2 = torch.exp(A) * u2 + net(u1, j, 'b')
            cols = [None] * 3
            for k, c in enumerate(i1):
                cols[c] = u1[:, k]
            for k, c in enumerate(i2):
                cols[c] = v2[:, k]
            u = torch.stack(cols, dim=1)
            ld = ld + A.sum(dim=1)
        llz = -0.5 * (u[:, :x_d] ** 2).sum(dim=1) - 0.5 * x_d * 1.8378770664093453
        lly = -lam * (u[:, x_d:] - xy[:, x_d:]).abs().sum(dim=1)
        return -(llz + lly + ld).mean()

    def step():
        loss = forward()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()

    def loss_now():
        with torch.no_grad():
            return float(forward())

    ms = _timed(torch, step, steps, warmup)
    return {'side': 'torch', 'step_ms': ms, 'loss': loss_now()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--side', choices=['hip', 'torch'])
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    a = ap.parse_args()
    if a.side:
        print(json.dumps((run_hip if a.side == 'hip' else run_torch)(a.steps, a.warmup)))
        return
    res = {'hip': [], 'torch': []}
    for _ in range(a.rounds):
        for side in ('hip', 'torch'):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--side', side, '--steps', str(a.steps),
                                '--warmup', str(a.warmup)], capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit(f'{side} run failed ({r.returncode}):\n{r.stdout}\n{r.stderr}')
            res[side].append(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps({'config': KW, 'B': B, 'steps': a.steps, 'warmup': a.warmup,
                      'hip_step_ms': [r['step_ms'] for r in res['hip']],
                      'torch_step_ms': [r['step_ms'] for r in res['torch']],
                      'hip_backward_ms': [r['backward_ms'] for r in res['hip']],
                      'loss_after': {'hip': res['hip'][-1]['loss'], 'torch': res['torch'][-1]['loss']}}))


if __name__ == '__main__':
    main()
