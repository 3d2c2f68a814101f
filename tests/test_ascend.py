"""cFlow.ascend / cnf_flow_ascend: Adam gradient ascent on the flow-input-space log-density llz + logdet over the
x channels of the flow's input, the condition fixed, in one native call.

The float64 side is the same ascent (Keras Adam, tests/test_train.adam_np with the gradient negated) under torch
autograd on oracle.cflow_torch_cpu.TorchCPUFlow, from the reference of tests/test_score.py. CPU tests: the argument
errors and that the committed learning rate makes the oracle's ascent a measurable climb. GPU tests: one step
against the by-hand update from cFlow.score's gradient, a run against its chained single steps, the climb against
the oracle's, and steps = 0."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from arl_conditional_normalizing_flows_amd import _lib
from oracle.cflow_torch_cpu import TorchCPUFlow
from test_score import A, FWD_RTOL, LOGIT_A, OUT, WS, X, Y, _capi_kw, _dev, _flow, _plan, log_density, refs
from test_train import adam_np

# The climb test's learning rate, chosen on the CPU: with it the float64 oracle's 20 Adam steps on tiny B = 3 raise
# every image's log-density by at least 100 x that image's forward bound 1e-5 max(|log_prob|, sum|s|)
# (test_oracle_ascent_climbs asserts it and prints the rises), so half the oracle's rise is far above what the
# fp32 forward's error could fake.
CLIMB_LR = 1e-2
CLIMB_STEPS = 20
ADAM = dict(beta_1=0.9, beta_2=0.999, epsilon=1e-7)


# ---------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------

def _desc(chunk=2, steps=3, lr=1e-2, beta_1=0.9, beta_2=0.999, epsilon=1e-7, logit_a=0.0, residual=0, first_step=0):
    return _lib.cnf_ascend_desc(chunk, steps, lr, beta_1, beta_2, epsilon, logit_a, residual, first_step)


def _call(lib, p, desc, plan=True, params=A, aux=A, x0=X, y=Y, x_out=OUT, trace=OUT + (1 << 30), m=None, v=None,
          ws=WS, B=3):
    return lib.cnf_flow_ascend(p if plan else None, params, aux, x0, y, C.byref(desc) if desc is not None else None,
                               x_out, trace, m, v, ws, B, None)


ARG_ERRORS = [
    ('null_plan', 'tiny', dict(plan=False), {}, 'null'),
    ('null_params', 'tiny', dict(params=None), {}, 'null'),
    ('null_aux', 'tiny', dict(aux=None), {}, 'null'),
    ('null_workspace', 'tiny', dict(ws=None), {}, 'null'),
    ('null_x0', 'tiny', dict(x0=None), {}, 'x0'),
    ('null_y', 'tiny', dict(y=None), {}, 'y'),
    ('null_x_out', 'tiny', dict(x_out=None), {}, 'x_out'),
    ('null_trace', 'tiny', dict(trace=None), {}, 'log_prob_trace'),
    ('m_without_v', 'tiny', dict(m=OUT + (2 << 30)), {}, 'together'),
    ('chunk', 'tiny', {}, dict(chunk=0), 'chunk'),
    ('steps', 'tiny', {}, dict(steps=-1), 'steps'),
    ('first_step', 'tiny', {}, dict(first_step=-1), 'first_step'),
    ('lr_nan', 'tiny', {}, dict(lr=float('nan')), 'lr'),
    ('lr_inf', 'tiny', {}, dict(lr=float('inf')), 'lr'),
    ('beta', 'tiny', {}, dict(beta_2=1.0), 'beta'),
    ('epsilon', 'tiny', {}, dict(epsilon=-1.0), 'epsilon'),
    ('logit_a_high', 'tiny', {}, dict(logit_a=0.5), 'logit_a'),
    ('residual_depth', 'small', {}, dict(residual=1), 'residual'),
    ('empty_batch', 'tiny', dict(B=0), {}, 'B'),
]


@pytest.mark.parametrize('what,preset,args,desc,word', ARG_ERRORS, ids=[e[0] for e in ARG_ERRORS])
def test_argument_errors(lib, what, preset, args, desc, word):
    """CNF_E_INVALID (-1) with the entry point's name and the argument in the message, before any HIP call."""
    p, keep = _plan(lib, _capi_kw(preset))
    try:
        assert _call(lib, p, _desc(**desc), **args) == -1
        msg = lib.cnf_last_error().decode()
        assert 'cnf_flow_ascend' in msg and word in msg, msg
        assert _call(lib, p, None) == -1
        msg = lib.cnf_last_error().decode()
        assert 'cnf_flow_ascend' in msg and 'descriptor' in msg, msg
    finally:
        lib.cnf_plan_destroy(p)


def test_valid_arguments_pass_the_check(lib):
    """The valid calls (steps = 0 and a caller's state among them) are not CNF_E_INVALID: without a device they
    stop at the first HIP call (CNF_E_HIP)."""
    if torch.cuda.is_available():
        return
    p, keep = _plan(lib, _capi_kw('tiny'))
    try:
        for d, args in ((_desc(), {}), (_desc(steps=0), {}), (_desc(logit_a=LOGIT_A, residual=1), {}),
                        (_desc(first_step=4), dict(m=OUT + (2 << 30), v=OUT + (3 << 30)))):
            assert _call(lib, p, d, **args) == -2, lib.cnf_last_error()
    finally:
        lib.cnf_plan_destroy(p)


@functools.lru_cache(maxsize=None)
def oracle_ascent(name='tiny', B=3, steps=CLIMB_STEPS, lr=CLIMB_LR):
    """float64: (trace [steps+1, B] of llz + logdet, forward bound [B] at the start) of the Adam ascent on x"""
    kw, P, x, y, _, _, _, _ = refs(name, B)
    tf = TorchCPUFlow(**kw)
    T = {k: torch.tensor(np.asarray(v, np.float64)) for k, v in P.items()}
    yt = torch.from_numpy(np.asarray(y, np.float64))
    u = np.asarray(x, np.float64)
    m, v = np.zeros_like(u), np.zeros_like(u)
    trace, bound = [], None
    for t in range(steps + 1):
        ut = torch.tensor(u, requires_grad=True)
        _, lp, abs_s = log_density(tf, T, ut, yt)
        trace.append(lp.detach().numpy().copy())
        if t == 0:
            bound = FWD_RTOL * np.maximum(np.abs(trace[0]), abs_s.detach().numpy())
        if t < steps:
            lp.sum().backward()
            u, m, v = adam_np(u, -ut.grad.numpy(), m, v, t + 1, lr=lr, b1=ADAM['beta_1'], b2=ADAM['beta_2'],
                              eps=ADAM['epsilon'])
    return np.stack(trace), bound


def test_oracle_ascent_climbs():
    """CLIMB_LR's condition: the oracle alone raises every image's log-density by >= 100 forward bounds."""
    trace, bound = oracle_ascent()
    rise = trace[-1] - trace[0]
    print(f'oracle rise {rise}, forward bound {bound}, rise / bound {rise / bound}')
    assert np.all(rise >= 100.0 * bound), (rise, bound)


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------

def bits(t):
    return t.contiguous().view(torch.int32)


def _logit(t, a, inverse):
    """cnf_logit on the device: the kernels' own logit_value / delogit_value"""
    out = torch.empty_like(t)
    assert _lib.load().cnf_logit(t.data_ptr(), out.data_ptr(), t.numel(), a, int(inverse),
                                 torch.cuda.current_stream().cuda_stream) == 0
    return out


def by_hand_step(flow, u0, y, chunk, lr):
    """u0 + alpha m / (sqrt(v) + eps) in torch fp32 from score's flow-space gradient at u0: k_ascend_step's
    operations in its order (Adam on -g from a zero state, step 1)"""
    f32 = lambda s: torch.tensor(s, dtype=torch.float32, device=u0.device)
    sc = flow.score(u0, y, chunk=chunk)
    b1, b2, eps = np.float32(ADAM['beta_1']), np.float32(ADAM['beta_2']), np.float32(ADAM['epsilon'])
    alpha = np.float32(float(np.float32(lr)) * np.sqrt(1.0 - float(b2)) / (1.0 - float(b1)))
    gi = -sc['grad_x']
    m = gi * f32(np.float32(1.0) - b1)
    v = (gi * gi) * f32(np.float32(1.0) - b2)
    return u0 - f32(alpha) * m / (torch.sqrt(v) + f32(eps)), sc['log_prob']


@pytest.mark.gpu
@pytest.mark.parametrize('name,B,chunk,transforms', [('tiny', 3, 2, False), ('small', 5, 2, False),
                                                     ('tiny', 3, 2, True)])
def test_one_step_by_hand(gpu, name, B, chunk, transforms):
    """ascend(steps=1) against the by-hand update, compared in flow space: per element within 16 ulp of lr plus
    1 ulp of |u| (a handful of fp32 roundings: the product contractions of the kernel).
    trace[0] is bit-equal to score's flow-space 'log_prob' at u0: both are k_score_seed's llz plus the same
    forward's log-det, and score's finish adds a log_jac of exactly 0 without the logit map.
    With the transforms, the flow-space start is u0 = logit_value(x0 - y) by cnf_logit (the gather's own
    expression): the call from x0 with the transforms must equal, bit for bit, the flow-space call from u0 taken
    through delogit_value and + y (the sampler's post-transform), and its trace that call's; the flow-space call
    is the one compared with the by-hand update."""
    lr = 1e-2
    r = refs(name, B, transforms)
    x, y = _dev(r, gpu)
    flow = _flow(r, gpu)
    u0 = _logit(x - y, LOGIT_A, 0) if transforms else x
    got = flow.ascend(u0, y, 1, lr=lr, chunk=chunk, **ADAM)
    hand, lp0 = by_hand_step(flow, u0, y, chunk, lr)
    assert got['log_prob'].shape == (2, B)
    assert torch.equal(bits(got['log_prob'][0]), bits(lp0))
    err = (got['x'].double() - hand.double()).abs().cpu().numpy()
    tol = 16.0 * float(np.spacing(np.float32(lr))) + np.spacing(np.abs(hand.cpu().numpy())).astype(np.float64)
    print(f'{name} one step: worst err/tol {np.max(err / tol):.3f}, max err {err.max():.3e}, '
          f'max |u1 - u0| {float((hand - u0).abs().max()):.3e}')
    assert np.all(err <= tol)
    assert float((got['x'] - u0).abs().max()) > 0.5 * lr   # (a step was taken: Adam's first step is ~ lr)
    if transforms:
        tr = flow.ascend(x, y, 1, lr=lr, chunk=chunk, logit_a=LOGIT_A, residual=True, **ADAM)
        assert torch.equal(bits(tr['log_prob']), bits(got['log_prob']))
        assert torch.equal(bits(tr['x']), bits(_logit(got['x'], LOGIT_A, 1) + y))


@pytest.mark.gpu
def test_chain(gpu):
    """ascend(steps=4) equals four chained ascend(steps=1, state=...) calls with the same chunk, bit for bit, in
    x, the trace and the state."""
    r = refs('small', 5)
    x, y = _dev(r, gpu)
    flow = _flow(r, gpu)
    whole = flow.ascend(x, y, 4, chunk=2, return_state=True)
    cur, state, rows = x, None, []
    for k in range(4):
        o = flow.ascend(cur, y, 1, chunk=2, state=state, return_state=True)
        rows.append(o['log_prob'][0])
        if k > 0:   # a call's start is the call before's end
            assert torch.equal(bits(o['log_prob'][0]), bits(last))
        cur, state, last = o['x'], o['state'], o['log_prob'][1]
    rows.append(last)
    assert state['step'] == whole['state']['step'] == 4
    assert torch.isfinite(whole['x']).all() and torch.isfinite(whole['log_prob']).all()
    assert torch.equal(bits(whole['x']), bits(cur))
    assert torch.equal(bits(whole['log_prob']), bits(torch.stack(rows)))
    for k in ('m', 'v'):
        assert torch.equal(bits(whole['state'][k]), bits(state[k])), k
    # the state in the workspace (no state asked for) is the same run
    plain = flow.ascend(x, y, 4, chunk=2)
    assert torch.equal(bits(plain['x']), bits(whole['x'])) and torch.equal(bits(plain['log_prob']), bits(whole['log_prob']))


@pytest.mark.gpu
def test_it_climbs(gpu):
    """tiny B = 3, CLIMB_STEPS steps at CLIMB_LR: every image's trace[-1] - trace[0] is at least half the float64
    oracle's rise, and cFlow.log_prob(x_out, y) (no transforms: llz + logdet) equals trace[-1] within the forward
    bound."""
    r = refs('tiny', 3)
    x, y = _dev(r, gpu)
    flow = _flow(r, gpu)
    ref_trace, bound0 = oracle_ascent()
    out = flow.ascend(x, y, CLIMB_STEPS, lr=CLIMB_LR, **ADAM)
    trace = out['log_prob'].cpu().numpy().astype(np.float64)
    rise, ref_rise = trace[-1] - trace[0], ref_trace[-1] - ref_trace[0]
    print(f'rise {rise}, oracle rise {ref_rise}, start err {np.abs(trace[0] - ref_trace[0])} (bound {bound0})')
    assert np.all(np.abs(trace[0] - ref_trace[0]) <= bound0)
    assert np.all(rise >= 0.5 * ref_rise), (rise, ref_rise)
    # the end point under the oracle: the bound at x_out
    kw, P = r[0], r[1]
    tf = TorchCPUFlow(**kw)
    T = {k: torch.tensor(np.asarray(v, np.float64)) for k, v in P.items()}
    _, lp, abs_s = log_density(tf, T, out['x'].cpu().double(), torch.from_numpy(np.asarray(r[3], np.float64)))
    bound = FWD_RTOL * np.maximum(np.abs(lp.numpy()), abs_s.numpy())
    again = flow.log_prob(out['x'], y)['log_prob'].cpu().numpy().astype(np.float64)
    print(f'log_prob(x_out) - trace[-1]: {again - trace[-1]}, bound {bound}')
    assert np.all(np.abs(again - trace[-1]) <= bound)
    assert np.all(np.abs(trace[-1] - lp.numpy()) <= bound)


@pytest.mark.gpu
@pytest.mark.parametrize('transforms', [False, True], ids=['plain', 'logit_residual'])
def test_zero_steps_and_y(gpu, transforms):
    """steps = 0: x is the post-transform of the gathered x0 (x0 itself without transforms, bit for bit; with
    them delogit_value(logit_value(x0 - y)) + y by the kernels' own expressions) and the trace has one row, the
    flow-space log-density of the start. y is never written, by steps = 0 or by a run."""
    r = refs('tiny', 3, transforms)
    x, y = _dev(r, gpu)
    y0, x0 = y.clone(), x.clone()
    flow = _flow(r, gpu)
    out = flow.ascend(x, y, 0, **r[4])
    assert out['log_prob'].shape == (1, 3) and torch.isfinite(out['log_prob']).all()
    want = _logit(_logit(x - y, LOGIT_A, 0), LOGIT_A, 1) + y if transforms else x
    assert torch.equal(bits(out['x']), bits(want))
    u0 = _logit(x - y, LOGIT_A, 0) if transforms else x
    assert torch.equal(bits(out['log_prob'][0]), bits(flow.score(u0, y)['log_prob']))
    run = flow.ascend(x, y, 3, **r[4])
    assert torch.equal(bits(out['log_prob'][0]), bits(run['log_prob'][0]))
    assert torch.equal(bits(y), bits(y0)) and torch.equal(bits(x), bits(x0))
    # an image outside the logit map's domain keeps its x and has -inf in every row; the others are untouched
    if transforms:
        xb = x.clone()
        xb[1, 2, 5, 0] = y[1, 2, 5, 0] - 1.0
        bad = flow.ascend(xb, y, 3, **r[4])
        assert torch.isinf(bad['log_prob'][:, 1]).all() and (bad['log_prob'][:, 1] < 0).all()
        assert torch.equal(bits(bad['x'][1]), bits(xb[1]))
        for i in (0, 2):
            assert torch.equal(bits(bad['x'][i]), bits(run['x'][i]))
            assert torch.equal(bits(bad['log_prob'][:, i]), bits(run['log_prob'][:, i]))
