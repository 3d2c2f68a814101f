"""cFlow.score / cnf_flow_score: the gradient of log_prob()['log_prob'] with respect to the image x and the
condition y, from the data-gradient-only backward.

Reference: torch autograd in float64 over oracle.cflow_torch_cpu.TorchCPUFlow.forward(xy, P, per_image=True), with
the gather's map restated here in torch (flow_space: v = x - y when residual, u = logit map of v, log_jac = the
sum over the x elements of log|du/dv|); x and y are leaves and (llz + logdet + log_jac).sum() is differentiated.
The CPU part checks that restatement against central finite differences, the symbols, the workspace sizes and the
argument errors, all without a GPU.

Bars (tests/test_train.py's, imported, none added). Each of grad_x, grad_y as one tensor:
  max|g - g_ref| <= K32 max|g32 - g_ref| + KP spread + GRAD_RTOL max|g_ref| + GRAD_ATOL gmax,
g32 the same graph in torch fp32, gmax the larger of max|grad_x_ref|, max|grad_y_ref|, spread (cfg2 only) the
float64 gradient's own movement under relative input perturbations PERTURB (PERTURB_SEEDS seeds each).
log_prob per image: |got - ref| <= 1e-5 max(|ref|, sum|s|), check_gradients' forward bound.
Weights init_params(5), inputs default_rng(6) / the synthetic batch of seed 6, as the other gradient tests."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from arl_conditional_normalizing_flows_amd import _lib
from arl_conditional_normalizing_flows_amd.config import PRESETS
from oracle.cflow_np import OracleCFlow
from oracle.cflow_torch_cpu import TorchCPUFlow
from test_train import GRAD_ATOL, GRAD_RTOL, K32, KP, PERTURB, PERTURB_SEEDS, _batch, _gpu_flow, _tol  # noqa: F401

LOG_2PI = float(np.log(2.0 * np.pi))
LOGIT_A = 0.01
FWD_RTOL = 1e-5   # check_gradients' forward bound: 1e-5 max(|ref|, sum|s|)

# ---------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------


def flow_space(x, y, logit_a=None, residual=False):
    """torch restatement of cnf_flow_log_prob's gather: (u, log_jac [B]) of x [B,H,W,x_d], y [B,H,W,D-x_d]:
    v = x - y (residual) or x; with logit_a e = a + (1 - 2a) v, u = (logit(e) - logit(a)) / span, span =
    logit(1 - a) - logit(a), and log_jac = sum log(du/dv) = sum log((1 - 2a) / (span e (1 - e)))."""
    v = x - y if residual else x
    if not logit_a:
        return v, torch.zeros(x.shape[0], dtype=x.dtype)
    a = float(logit_a)
    c1 = 1.0 - 2.0 * a
    lo = float(np.log(a / (1.0 - a)))
    span = float(np.log((1.0 - a) / a)) - lo
    e = a + c1 * v
    u = (torch.log(e) - torch.log1p(-e) - lo) / span
    lj = (np.log(c1) - np.log(span) - torch.log(e) - torch.log1p(-e)).reshape(x.shape[0], -1).sum(1)
    return u, lj


def log_density(tf, T, x, y, logit_a=None, residual=False):
    """(log_prob [B], flow-space llz + logdet [B], sum|s| [B]) of the torch flow tf with weights T"""
    x_d = x.shape[-1]
    u, lj = flow_space(x, y, logit_a, residual)
    zy, ld = tf.forward(torch.cat([u, y], -1), T, per_image=True)
    z = zy[..., :x_d]
    llz = (-0.5 * (z * z).sum(-1) - 0.5 * x_d * LOG_2PI).reshape(x.shape[0], -1).sum(1)
    return llz + ld[0] + lj, llz + ld[0], ld[1]


def oracle_score(kw, P, x, y, logit_a=None, residual=False, dtype=torch.float64):
    """autograd: (grad_x, grad_y, log_prob, sum|s|) as float64 arrays"""
    tf = TorchCPUFlow(**kw)
    T = {k: torch.tensor(np.asarray(v, np.float64), dtype=dtype) for k, v in P.items()}
    xt = torch.tensor(np.asarray(x, np.float64), dtype=dtype, requires_grad=True)
    yt = torch.tensor(np.asarray(y, np.float64), dtype=dtype, requires_grad=True)
    lp, _, abs_s = log_density(tf, T, xt, yt, logit_a, residual)
    lp.sum().backward()
    f = lambda t: t.detach().double().numpy().copy()
    return f(xt.grad), f(yt.grad), f(lp), f(abs_s)


def inputs(name, B, transforms=False):
    """fp32 (x, y) of the synthetic batch of seed 6; with the transforms x = y + r, r uniform in (0.05, 0.95)
    from default_rng(6), so that x - y lies inside the logit map's domain"""
    cfg = PRESETS[name]
    xy = _batch(cfg, B, 6)
    x, y = np.ascontiguousarray(xy[..., :cfg.x_d]), np.ascontiguousarray(xy[..., cfg.x_d:])
    if transforms:
        x = (y + np.random.default_rng(6).uniform(0.05, 0.95, x.shape)).astype(np.float32)
    return x.astype(np.float32), y.astype(np.float32)


def weights(name, kw, regime):
    ora = OracleCFlow(**kw)
    if regime is None:
        return ora.init_params(5)
    from test_value_regimes import regime_params
    return regime_params(ora, regime)


@functools.lru_cache(maxsize=None)
def refs(name, B, transforms=False, layer_norm=True, regime=None):
    """(kw, P, x, y, opts, (gx, gy, lp, abs_s) float64, (gx32, gy32), (spread_x, spread_y)): computed once per
    case and shared by the tests (never modified)"""
    kw = dict(PRESETS[name].kwargs(), LAYER_NORM=layer_norm)
    P = weights(name, kw, regime)
    x, y = inputs(name, B, transforms)
    opts = dict(logit_a=LOGIT_A, residual=True) if transforms else {}
    ref = oracle_score(kw, P, x, y, **opts)
    g32 = oracle_score(kw, P, x, y, dtype=torch.float32, **opts)[:2]
    spread = [0.0, 0.0]
    if name == 'cfg2':   # the float64 gradient's own spread under perturbations of the fp32 forward's rounding size
        rng = np.random.default_rng(11)
        for eps in PERTURB:
            for _ in range(PERTURB_SEEDS):
                xp = np.asarray(x, np.float64) * (1.0 + eps * rng.standard_normal(x.shape))
                yp = np.asarray(y, np.float64) * (1.0 + eps * rng.standard_normal(y.shape))
                gp = oracle_score(kw, P, xp, yp, **opts)
                for i in range(2):
                    spread[i] = max(spread[i], float(np.max(np.abs(gp[i] - ref[i]))))
    return kw, P, x, y, opts, ref, g32, tuple(spread)


def check_score(out, r, what):
    """the module docstring's bars on a score() result (or its rows `sel` of the case's batch)"""
    kw, P, x, y, opts, (gx, gy, lp, abs_s), (gx32, gy32), spread = r
    gmax = max(float(np.max(np.abs(gx))), float(np.max(np.abs(gy))))
    got_lp = out['log_prob'].cpu().numpy().astype(np.float64)
    bound = FWD_RTOL * np.maximum(np.abs(lp), abs_s)
    print(f'{what} log_prob: worst err/bound {np.max(np.abs(got_lp - lp) / bound):.3f}')
    assert np.all(np.abs(got_lp - lp) <= bound), (what, got_lp, lp, bound)
    for key, ref, g32, sp in (('grad_x', gx, gx32, spread[0]), ('grad_y', gy, gy32, spread[1])):
        got = out[key].cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all(), (what, key)
        err = float(np.max(np.abs(got - ref)))
        tol = _tol(ref, g32, gmax) + KP * sp
        print(f'{what} {key}: max|dg| {err:.3e}, tol {tol:.3e} (err/tol {err / tol:.3f}; max|g_ref| '
              f'{np.max(np.abs(ref)):.3e}, fp32 autograd err {np.max(np.abs(g32 - ref)):.3e}, spread {sp:.3e})')
        assert err <= tol, (what, key, err, tol)


# ---------------------------------------------------------------------------------------------
# CPU: the C ABI's host side and the reference itself
# ---------------------------------------------------------------------------------------------

A, X, Y, WS, OUT = 1 << 40, 2 << 40, 3 << 40, 4 << 40, 5 << 40   # placeholder device addresses, never dereferenced


def _capi_kw(name):
    kw = PRESETS[name].kwargs()
    kw.pop('group_mode')
    return kw


def _plan(lib, kw):
    arr = lambda v: (C.c_int * len(v))(*v)
    keep = [arr(kw['squeeze_factor_block_list']), arr(kw['ResNeXt_block_list']), arr(kw['num_kernels_list']),
            arr(kw['cardinality_list'])]
    d = _lib.cnf_flow_desc(*kw['io_shape'], kw['x_d'], len(keep[0]), *keep, float(kw.get('lambda_y', 100.0)), 3,
                           int(kw.get('LAYER_NORM', True)), int(kw.get('DILATIONS', True)), 0, None)
    p = C.c_void_p()
    rc = lib.cnf_plan_create(C.byref(d), C.byref(p))
    assert rc == 0, lib.cnf_last_error()
    return p, keep


def _desc(chunk=2, logit_a=0.0, residual=0):
    return _lib.cnf_score_desc(chunk, logit_a, residual)


def _call(lib, p, desc, plan=True, params=A, aux=A, x=X, y=Y, grad_x=OUT, grad_y=OUT + (1 << 30),
          log_prob=OUT + (2 << 30), ws=WS, B=3):
    return lib.cnf_flow_score(p if plan else None, params, aux, x, y, C.byref(desc) if desc is not None else None,
                              grad_x, grad_y, log_prob, ws, B, None)


def test_symbols_exist(lib):
    for s in ('cnf_plan_score_workspace_bytes', 'cnf_flow_score', 'cnf_plan_ascend_workspace_bytes',
              'cnf_flow_ascend'):
        assert hasattr(lib, s) and s in _lib.EXPORTED_SYMBOLS, s
    assert lib.cnf_version() != b'cnf-mi355x 0.1 (gfx950)' and b'gfx950' in lib.cnf_version()


# (what to change in a valid call on `preset`, a word of the message)
ARG_ERRORS = [
    ('null_plan', 'tiny', dict(plan=False), {}, 'null'),
    ('null_params', 'tiny', dict(params=None), {}, 'null'),
    ('null_aux', 'tiny', dict(aux=None), {}, 'null'),
    ('null_workspace', 'tiny', dict(ws=None), {}, 'null'),
    ('null_x', 'tiny', dict(x=None), {}, 'x'),
    ('null_y', 'tiny', dict(y=None), {}, 'y'),
    ('no_output', 'tiny', dict(grad_x=None, grad_y=None, log_prob=None), {}, 'output'),
    ('chunk', 'tiny', {}, dict(chunk=0), 'chunk'),
    ('logit_a_high', 'tiny', {}, dict(logit_a=0.5), 'logit_a'),
    ('logit_a_negative', 'tiny', {}, dict(logit_a=-0.1), 'logit_a'),
    ('residual_depth', 'small', {}, dict(residual=1), 'residual'),
    ('empty_batch', 'tiny', dict(B=0), {}, 'B'),
]


@pytest.mark.parametrize('what,preset,args,desc,word', ARG_ERRORS, ids=[e[0] for e in ARG_ERRORS])
def test_argument_errors(lib, what, preset, args, desc, word):
    """CNF_E_INVALID (-1) with the entry point's name and the argument in the message, before any HIP call: no GPU
    is needed and the placeholder addresses are never dereferenced."""
    p, keep = _plan(lib, _capi_kw(preset))
    try:
        assert _call(lib, p, _desc(**desc), **args) == -1
        msg = lib.cnf_last_error().decode()
        assert 'cnf_flow_score' in msg and word in msg, msg
        assert _call(lib, p, None) == -1
        msg = lib.cnf_last_error().decode()
        assert 'cnf_flow_score' in msg and 'descriptor' in msg, msg
    finally:
        lib.cnf_plan_destroy(p)


def test_valid_arguments_pass_the_check(lib):
    """The valid call of ARG_ERRORS, and each subset of the outputs, is not CNF_E_INVALID: without a device it stops
    at its first HIP call (CNF_E_HIP). On a device the GPU tests make the valid calls, on real buffers."""
    if torch.cuda.is_available():
        return
    p, keep = _plan(lib, _capi_kw('tiny'))
    try:
        for d, args in ((_desc(), {}), (_desc(logit_a=LOGIT_A, residual=1), {}), (_desc(), dict(grad_y=None)),
                        (_desc(), dict(grad_x=None, grad_y=None)), (_desc(), dict(log_prob=None, grad_x=None))):
            assert _call(lib, p, d, **args) == -2, lib.cnf_last_error()
    finally:
        lib.cnf_plan_destroy(p)


@pytest.mark.parametrize('name', ['tiny', 'small', 'cfg2'])
def test_workspaces(lib, name):
    """cnf_plan_score_workspace_bytes and cnf_plan_ascend_workspace_bytes: more than the train workspace of
    `chunk` images, the same for every B, monotone in chunk; 0 with a message naming the function otherwise."""
    p, keep = _plan(lib, _capi_kw(name))
    try:
        ad = lambda chunk, steps=3: _lib.cnf_ascend_desc(chunk, steps, 1e-2, 0.9, 0.999, 1e-7, 0.0, 0, 0)
        prev = (0, 0)
        for chunk in (1, 2, 7, 64):
            train = int(lib.cnf_plan_train_workspace_bytes(p, chunk))
            sc = {B: int(lib.cnf_plan_score_workspace_bytes(p, B, C.byref(_desc(chunk)))) for B in (1, 5, 1000)}
            asc = {B: int(lib.cnf_plan_ascend_workspace_bytes(p, B, C.byref(ad(chunk)))) for B in (1, 5, 1000)}
            assert len(set(sc.values())) == 1 and len(set(asc.values())) == 1, (sc, asc)
            assert asc[1] > sc[1] > train > 0, (name, chunk, asc[1], sc[1], train)
            assert sc[1] > prev[0] and asc[1] > prev[1], (name, chunk)
            prev = (sc[1], asc[1])
        for bad, word in ((_desc(0), 'chunk'), (_desc(2, 0.7), 'logit_a')):
            assert lib.cnf_plan_score_workspace_bytes(p, 2, C.byref(bad)) == 0
            msg = lib.cnf_last_error().decode()
            assert 'cnf_plan_score_workspace_bytes' in msg and word in msg, msg
        assert lib.cnf_plan_score_workspace_bytes(p, 0, C.byref(_desc())) == 0
        assert lib.cnf_plan_score_workspace_bytes(p, 2, None) == 0
        assert lib.cnf_plan_score_workspace_bytes(None, 2, C.byref(_desc())) == 0
        for bad, word in ((ad(0), 'chunk'), (ad(2, -1), 'steps')):
            assert lib.cnf_plan_ascend_workspace_bytes(p, 2, C.byref(bad)) == 0
            msg = lib.cnf_last_error().decode()
            assert 'cnf_plan_ascend_workspace_bytes' in msg and word in msg, msg
    finally:
        lib.cnf_plan_destroy(p)


@pytest.mark.parametrize('transforms', [False, True], ids=['plain', 'logit_residual'])
def test_reference_matches_finite_differences(transforms):
    """The torch restatement of the logit / residual / log_jac chain in front of the oracle flow, differentiated
    by autograd, against central differences of the same float64 function on `tiny`, at random elements of x and
    of y (as test_train.test_oracle_gradient_matches_finite_differences does for parameters)."""
    kw, P, x, y, opts, (gx, gy, lp, _), _, _ = refs('tiny', 2, transforms)
    tf = TorchCPUFlow(**kw)
    T = {k: torch.tensor(np.asarray(v, np.float64)) for k, v in P.items()}
    x64, y64 = np.asarray(x, np.float64), np.asarray(y, np.float64)

    def f(xa, ya):
        return float(log_density(tf, T, torch.from_numpy(xa), torch.from_numpy(ya), **opts)[0].sum())

    rng = np.random.default_rng(0)
    eps = 1e-6
    for which, g in (('x', gx), ('y', gy)):
        for _ in range(6):
            idx = tuple(int(rng.integers(0, s)) for s in g.shape)
            ap, am = [x64.copy(), y64.copy()], [x64.copy(), y64.copy()]
            k = 0 if which == 'x' else 1
            ap[k][idx] += eps
            am[k][idx] -= eps
            fd = (f(*ap) - f(*am)) / (2 * eps)
            assert abs(fd - g[idx]) <= 1e-4 * max(1.0, abs(g[idx])), (which, idx, fd, g[idx])


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------

def _flow(r, gpu, options=None):
    return _gpu_flow(r[0], r[1], gpu, options)


def _dev(r, gpu):
    return torch.from_numpy(r[2]).to(gpu), torch.from_numpy(r[3]).to(gpu)


# (preset, B, transforms, LAYER_NORM, weight regime, debug options): every backward path in data-only mode at the
# smallest shape that reaches it
SCORE_CASES = [
    ('tiny', 2, False, True, None, None),
    ('tiny', 2, True, True, None, None),
    ('small', 3, False, True, None, None),
    ('small', 3, False, True, None, {'LDS_BWD': 0}),
    ('small', 3, False, True, None, {'LDS_BWD': 1}),
    ('small', 3, False, True, None, {'TRAIN_ALT': 1}),
    ('small', 3, False, True, None, {'NETLDS': 0}),
    ('narrow', 3, False, True, None, None),
    ('cfg2', 2, False, True, None, None),
    ('tiny', 2, False, False, None, None),
    # tanh and the LeakyReLU slopes away from initialisation (tests/test_value_regimes.py 'trained')
    ('small', 3, False, True, 'trained', None),
]


@pytest.mark.gpu
@pytest.mark.parametrize('name,B,transforms,ln,regime,options', SCORE_CASES,
                         ids=['-'.join(str(v) for v in c) for c in SCORE_CASES])
def test_score_matches_oracle(gpu, name, B, transforms, ln, regime, options):
    r = refs(name, B, transforms, ln, regime)
    x, y = _dev(r, gpu)
    out = _flow(r, gpu, options).score(x, y, return_grad_y=True, **r[4])
    check_score(out, r, f'{name} B={B} {r[4]} {options} {regime}')
    assert set(out) == {'grad_x', 'grad_y', 'log_prob'}


@pytest.mark.gpu
def test_ragged_chunks(gpu):
    """small, B = 5, chunk 1, 2 (a ragged last chunk) and 5: each under the oracle bars, 'log_prob' bit-equal
    across the three. The gradients are not required to be: k_tconv_band's tile height follows the launch's
    workgroup count, which counts the chunk's images (cFlow.score's docstring)."""
    r = refs('small', 5)
    x, y = _dev(r, gpu)
    flow = _flow(r, gpu)
    outs = {c: flow.score(x, y, chunk=c, return_grad_y=True) for c in (1, 2, 5)}
    for c, o in outs.items():
        check_score(o, r, f'small B=5 chunk={c}')
    for c in (2, 5):
        assert torch.equal(outs[1]['log_prob'].view(torch.int32), outs[c]['log_prob'].view(torch.int32)), c
        for k in ('grad_x', 'grad_y'):
            d = float((outs[1][k] - outs[c][k]).abs().max())
            print(f'chunk 1 vs {c} {k}: max abs diff {d:.3e}')


@pytest.mark.gpu
def test_domain(gpu):
    """One image of three with an element outside the logit map's domain: its log_prob is -inf and its gradients
    NaN; the other two images equal, bit for bit, the same call with that element inside the domain."""
    r = refs('tiny', 3, True)
    x, y = _dev(r, gpu)
    flow = _flow(r, gpu)
    good = flow.score(x, y, return_grad_y=True, **r[4])
    xb = x.clone()
    xb[1, 3, 4, 0] = y[1, 3, 4, 0] + 2.0
    bad = flow.score(xb, y, return_grad_y=True, **r[4])
    assert float(bad['log_prob'][1]) == float('-inf')
    assert torch.isnan(bad['grad_x'][1]).all() and torch.isnan(bad['grad_y'][1]).all()
    for i in (0, 2):
        for k in ('grad_x', 'grad_y', 'log_prob'):
            assert torch.isfinite(bad[k][i]).all(), (i, k)
            assert torch.equal(bad[k][i].contiguous().view(torch.int32), good[k][i].contiguous().view(torch.int32)), (i, k)


G = 1 << 20   # guard band bytes on either side of a payload (tests/test_state_independence.py's pattern)


def guarded(nbytes, fill):
    """(payload, check): a uint8 payload of nbytes filled with `fill` inside a slab whose guard bands hold the
    complement; check() synchronises and asserts that no guard byte changed"""
    nbytes = int(nbytes)
    guard = 0xFF ^ fill
    slab = torch.empty(G + nbytes + G, device='cuda', dtype=torch.uint8)
    slab[:G].fill_(guard)
    slab[G + nbytes:].fill_(guard)
    payload = slab[G:G + nbytes]
    payload.fill_(fill)

    def check(what=''):
        torch.cuda.synchronize()
        for side, band in (('below', slab[:G]), ('above', slab[G + nbytes:])):
            bad = torch.nonzero(band != guard).flatten()
            assert bad.numel() == 0, f'{what}: {bad.numel()} guard bytes {side} the buffer changed'
    return payload, check


@pytest.mark.gpu
def test_state_independence(gpu):
    """cnf_flow_score through the C ABI (small, B = 3, chunk 2: a ragged chunk) on a guarded workspace and
    guarded outputs pre-filled with zeros (Z) and with 0xFF (N: NaN): the outputs are finite and bit-equal, no
    guard byte changes; and the same call on two other streams gives the same bits."""
    r = refs('small', 3)
    x, y = _dev(r, gpu)
    flow = _flow(r, gpu)
    lib = _lib.load()
    desc = _lib.cnf_score_desc(2, 0.0, 0)
    nws = int(lib.cnf_plan_score_workspace_bytes(flow._plan, 3, C.byref(desc)))
    assert nws > 0
    sizes = {'grad_x': x.numel() * 4, 'grad_y': y.numel() * 4, 'log_prob': 3 * 4}

    def run(fill, stream=None):
        ws, ck = guarded(nws, fill)
        bufs = {k: guarded(n, fill) for k, n in sizes.items()}
        st = stream if stream is not None else torch.cuda.current_stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            rc = lib.cnf_flow_score(flow._plan, flow.params.data_ptr(), flow._aux.data_ptr(), x.data_ptr(),
                                    y.data_ptr(), C.byref(desc), bufs['grad_x'][0].data_ptr(),
                                    bufs['grad_y'][0].data_ptr(), bufs['log_prob'][0].data_ptr(), ws.data_ptr(), 3,
                                    st.cuda_stream)
        assert rc == 0, lib.cnf_last_error()
        ck(f'workspace fill {fill:#x}')
        for k, (_, c) in bufs.items():
            c(f'{k} fill {fill:#x}')
        return {k: b.view(torch.float32).clone() for k, (b, _) in bufs.items()}

    z, n = run(0x00), run(0xFF)
    s1, s2 = run(0x00, torch.cuda.Stream()), run(0xFF, torch.cuda.Stream())
    for k in sizes:
        assert torch.isfinite(z[k]).all(), k
        for other, what in ((n, 'N'), (s1, 'stream 1'), (s2, 'stream 2')):
            assert torch.equal(z[k].view(torch.int32), other[k].view(torch.int32)), (k, what)


@pytest.mark.gpu
def test_training_gradients_untouched(gpu):
    """flow.gradients(xy) before and after a score and an ascend call on the same flow: the same bits (no plan
    state leaks: the event pool, the side streams, the dense backward image)."""
    r = refs('small', 3)
    x, y = _dev(r, gpu)
    xy = torch.cat([x, y], -1).contiguous()
    flow = _flow(r, gpu)
    g0 = flow.gradients(xy)[0].clone()
    flow.score(x, y, chunk=2, return_grad_y=True)
    flow.ascend(x, y, steps=2, chunk=2)
    g1 = flow.gradients(xy)[0].clone()
    torch.cuda.synchronize()
    assert torch.isfinite(g0).all()
    assert torch.equal(g0.view(torch.int32), g1.view(torch.int32))
