"""cFlow.log_prob / cnf_flow_log_prob (include/cnf.h): the density of given images in the space of the samples,
per (image, condition) pair, with the class posterior.

CPU part (host only): every argument error is CNF_E_INVALID with its message before any HIP call, the workspace
does not scale with B or K, and the forward's dry-run schedule is what it was before flow_forward learnt to
append to a recording.

GPU part, on tiny (8x8x2, x_d 1) and small (16x16x4, x_d 3) with B = 3 images and K = 5 conditions: every
returned term against the float64 oracle under the project's bound (below), on synthetic images and on the
model's own draws; pairwise == paired on the expanded pairs, no dependence on chunk, the workspace's contents,
the stream or a relaunch, all bit for bit; the posterior against float64; the logit map's domain edge; the
Python surface.

Bounds (written before the first GPU run). With ref terms llz, ld, lj of the float64 oracle at the float64
flow-space image of the same fp32 x and y, q = sum z^2, S = sum |s| over the couplings, T = sum |log_jac terms|:
  log_prob  1e-5 max(|llz| + |ld| + |lj|, 0.5 q + S + T)   (log_prob_oracle's form + the Jacobian's scale)
  llz       1e-5 max(|llz|, 0.5 q);   logdet  1e-5 max(|ld|, S);   log_jac  1e-5 max(|lj|, T), exactly 0 without
            the map
  y_dev     1e-5 * (number of y elements) * max|zy_ref|: the forward's parity bound per element (1e-5 of the
            tensor's largest magnitude, tests/test_gpu_parity.py), once per |.| of the sum

_setup / _plan / log_prob_oracle's form and the 'trained' weight regime are tests/test_inverse_logdet.py's,
restated here."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from arl_conditional_normalizing_flows_amd import _lib
from arl_conditional_normalizing_flows_amd.config import PRESETS
from oracle.cflow_np import OracleCFlow, synthetic_class_batch, synthetic_sr_batch
from oracle.transforms_np import de_logitify, logit_preprocess

RTOL = 1e-5
LOG_2PI = float(np.log(2.0 * np.pi))
B_IMG, K_COND = 3, 5
LOGIT_A = 0.01

# ---------------------------------------------------------------------------------------------
# CPU: the C ABI's host side
# ---------------------------------------------------------------------------------------------

A, X, Y, WS, OUT = 1 << 40, 2 << 40, 3 << 40, 4 << 40, 5 << 40   # placeholder device addresses, never dereferenced


def _capi_kw(name):
    kw = PRESETS[name].kwargs()
    kw.pop('group_mode')
    return kw


def _plan(lib, kw, group_mode=0, options=None):
    arr = lambda v: (C.c_int * len(v))(*v)
    keep = [arr(kw['squeeze_factor_block_list']), arr(kw['ResNeXt_block_list']), arr(kw['num_kernels_list']),
            arr(kw['cardinality_list'])]
    d = _lib.cnf_flow_desc(*kw['io_shape'], kw['x_d'], len(keep[0]), *keep, float(kw.get('lambda_y', 100.0)), 3,
                           int(kw.get('LAYER_NORM', True)), int(kw.get('DILATIONS', True)), group_mode,
                           options.encode() if options else None)
    p = C.c_void_p()
    rc = lib.cnf_plan_create(C.byref(d), C.byref(p))
    return rc, p, keep


def _desc(K=5, chunk=4, logit_a=0.0, residual=0):
    return _lib.cnf_logp_desc(K, chunk, logit_a, residual)


def _call(lib, p, desc, plan=True, params=A, aux=A, x=X, y=Y, log_prob=OUT, llz=None, logdet=None, log_jac=None,
          y_dev=None, log_prior=None, posterior=None, log_evidence=None, ws=WS, B=3):
    return lib.cnf_flow_log_prob(p if plan else None, params, aux, x, y, C.byref(desc) if desc is not None else None,
                                 log_prob, llz, logdet, log_jac, y_dev, log_prior, posterior, log_evidence, ws, B,
                                 None)


# (what to change in a valid pairwise call on `preset`, a word of the message)
ARG_ERRORS = [
    ('null_plan', 'tiny', dict(plan=False), {}, 'null'),
    ('null_params', 'tiny', dict(params=None), {}, 'null'),
    ('null_aux', 'tiny', dict(aux=None), {}, 'null'),
    ('null_workspace', 'tiny', dict(ws=None), {}, 'null'),
    ('null_x', 'tiny', dict(x=None), {}, 'x'),
    ('null_y', 'tiny', dict(y=None), {}, 'y'),
    ('no_output', 'tiny', dict(log_prob=None), {}, 'output'),
    ('chunk', 'tiny', {}, dict(chunk=0), 'chunk'),
    ('logit_a_high', 'tiny', {}, dict(logit_a=0.5), 'logit_a'),
    ('logit_a_negative', 'tiny', {}, dict(logit_a=-0.1), 'logit_a'),
    ('residual_depth', 'small', {}, dict(residual=1), 'residual'),
    ('posterior_paired', 'tiny', dict(posterior=OUT + (1 << 30)), dict(K=0), 'posterior'),
    ('evidence_paired', 'tiny', dict(log_evidence=OUT + (1 << 30)), dict(K=0), 'posterior'),
    ('prior_without_posterior', 'tiny', dict(log_prior=OUT + (2 << 30)), {}, 'log_prior'),
    ('negative_K', 'tiny', {}, dict(K=-1), 'num_conditions'),
    ('empty_batch', 'tiny', dict(B=0), {}, 'B'),
]


@pytest.mark.parametrize('what,preset,args,desc,word', ARG_ERRORS, ids=[e[0] for e in ARG_ERRORS])
def test_argument_errors(lib, what, preset, args, desc, word):
    """CNF_E_INVALID (-1) with a message naming the argument, before any HIP call: no GPU is needed and the
    placeholder addresses are never dereferenced."""
    rc, p, keep = _plan(lib, _capi_kw(preset))
    assert rc == 0, lib.cnf_last_error()
    try:
        assert _call(lib, p, _desc(**desc), **args) == -1
        msg = lib.cnf_last_error().decode()
        assert 'cnf_flow_log_prob' in msg and word in msg, msg
        assert _call(lib, p, None) == -1 and 'descriptor' in lib.cnf_last_error().decode()
    finally:
        lib.cnf_plan_destroy(p)


def test_valid_arguments_pass_the_check(lib):
    """The valid call of ARG_ERRORS is not CNF_E_INVALID: without a device it stops at its first HIP call
    (CNF_E_HIP), placeholder addresses untouched; residual on tiny (D - x_d == x_d) passes too. On a device the
    GPU tests below make the valid calls, on real buffers."""
    if torch.cuda.is_available():
        return
    rc, p, keep = _plan(lib, _capi_kw('tiny'))
    assert rc == 0, lib.cnf_last_error()
    try:
        for d in (_desc(), _desc(K=0), _desc(logit_a=LOGIT_A, residual=1)):
            assert _call(lib, p, d) == -2, lib.cnf_last_error()
    finally:
        lib.cnf_plan_destroy(p)


@pytest.mark.parametrize('name', ['tiny', 'small', 'cfg2'])
def test_workspace_does_not_scale_with_pairs(lib, name):
    """cnf_plan_logp_workspace_bytes: the forward workspace of one chunk plus one chunk each of xy, zy, the
    log-det and the log_jac partials, whatever B and K; 0 with a message for a bad descriptor."""
    kw = _capi_kw(name)
    H, W, D = kw['io_shape']
    rc, p, keep = _plan(lib, kw)
    assert rc == 0, lib.cnf_last_error()
    try:
        for chunk in (1, 7, 64):
            parts = -(-H * W // 1024)
            need = int(lib.cnf_plan_workspace_bytes(p, chunk)) + chunk * (2 * H * W * D * 4 + 4 + 8 * parts)
            got = {(B, K): int(lib.cnf_plan_logp_workspace_bytes(p, B, C.byref(_desc(K=K, chunk=chunk))))
                   for B in (1, 1000) for K in (0, 1, 10, 1000)}
            assert len(set(got.values())) == 1, got
            assert need <= got[(1, 0)] <= need + 5 * 256, (name, chunk, got[(1, 0)], need)
        for bad, word in ((_desc(chunk=0), 'chunk'), (_desc(logit_a=0.7), 'logit_a'), (_desc(K=-2), 'num_conditions')):
            assert lib.cnf_plan_logp_workspace_bytes(p, 2, C.byref(bad)) == 0
            msg = lib.cnf_last_error().decode()
            assert 'cnf_plan_logp_workspace_bytes' in msg and word in msg, msg
        assert lib.cnf_plan_logp_workspace_bytes(p, 0, C.byref(_desc())) == 0
        assert lib.cnf_plan_logp_workspace_bytes(p, 2, None) == 0
        assert lib.cnf_plan_logp_workspace_bytes(None, 2, C.byref(_desc())) == 0
    finally:
        lib.cnf_plan_destroy(p)


# the forward's launches (cnf_debug_schedule, direction +1) of the commit before flow_forward's append option
FORWARD_SCHEDULE = {
    'tiny': ['k_net_lds'] * 8 + ['k_map2', 'k_map2'],
    'small': ['k_net_lds'] * 8 + ['k_map2'] + ['k_net_lds'] * 4 + ['k_map2'],
}


@pytest.mark.parametrize('name', list(FORWARD_SCHEDULE))
def test_forward_schedule_is_unchanged(lib, name):
    """flow_forward's append option is off by default: the dry run of the forward lists the launches it listed
    before, at every batch, and a second dry run starts from an empty recording."""
    lib.cnf_debug_schedule.restype = C.c_int
    lib.cnf_debug_schedule.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_int]
    rc, p, keep = _plan(lib, _capi_kw(name))
    assert rc == 0, lib.cnf_last_error()
    try:
        for B in (1, 3, 3):
            buf = C.create_string_buffer(1 << 16)
            n = lib.cnf_debug_schedule(p, B, 1, buf, 1 << 16)
            assert n > 0, lib.cnf_last_error()
            assert buf.value.decode().split('\n')[:-1] == FORWARD_SCHEDULE[name]
            assert lib.cnf_plan_num_recorded_launches(p) == 0
    finally:
        lib.cnf_plan_destroy(p)


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------

def _batch(name, B, seed):
    cfg = PRESETS[name]
    H, W, _D = cfg.io_shape
    if cfg.data == 'class':
        return synthetic_class_batch(B, H, W, cfg.x_d, seed=seed)
    return synthetic_sr_batch(B, H, W, cfg.x_d, cfg.sr_pow, seed=seed)


def _trained(P):
    """every parameter kind as after some epochs (tests/test_value_regimes.py 'trained'): kernels x3 (x8 on
    conv_out), bias ~ N(0, 0.3), gamma = 1 + N(0, 0.5), beta ~ N(0, 0.5), tanh_scale.w = 2; as fp32 values"""
    rng = np.random.default_rng(9)
    out = {}
    for k, v in P.items():
        v = np.asarray(v, np.float64)
        if k.endswith('.kernel'):
            v = v * (8.0 if '.conv_out.' in k else 3.0)
        elif k.endswith('.bias'):
            v = rng.normal(0, 0.3, v.shape)
        elif k.endswith('.gamma'):
            v = 1.0 + rng.normal(0, 0.5, v.shape)
        elif k.endswith('.beta'):
            v = rng.normal(0, 0.5, v.shape)
        elif k.endswith('.w'):
            v = np.asarray(2.0)
        out[k] = np.asarray(np.asarray(v, np.float32), np.float64)
    return out


@functools.lru_cache(maxsize=None)
def _setup(name, regime='init'):
    """(flow, oracle, weights): one flow per preset and weight regime for the whole file"""
    from arl_conditional_normalizing_flows_amd.make_model import cFlow
    kw = PRESETS[name].kwargs()
    flow = cFlow(**kw, debug_options={'NETLDS': 1})
    ora = OracleCFlow(**kw)
    P = ora.init_params(0)
    if regime == 'trained':
        P = _trained(ora.init_params(2))
    flow.set_weights(P)
    return flow, ora, P


MODES = {'plain': dict(), 'logit': dict(logit_a=LOGIT_A), 'residual': dict(residual=True)}


@functools.lru_cache(maxsize=None)
def _inputs(name, mode):
    """fp32 (x [B,H,W,x_d] in sample space, y [K,H,W,D-x_d]) from the synthetic batches: the x channels of one
    batch as the flow-space images, through de_logitify (logit) or + the batch's own y (residual)"""
    x_d = PRESETS[name].x_d
    xb = _batch(name, B_IMG, 1).astype(np.float64)
    y = np.ascontiguousarray(_batch(name, K_COND, 5)[..., x_d:])
    x = xb[..., :x_d]
    if mode == 'logit':
        x = de_logitify(x, LOGIT_A)
    if mode == 'residual':
        x = x + xb[..., x_d:]
    return np.ascontiguousarray(x.astype(np.float32)), y


def log_prob_reference(ora, P, x, y, logit_a=None, residual=False):
    """float64 terms and bounds of paired inputs x [n,H,W,x_d], y [n,H,W,D-x_d] (fp32 values): v by the oracle's
    logit_preprocess of x - y, the oracle's forward of concat(v, y), log N(z; 0, I) and the closed-form
    log-Jacobian. Returns ({term: ref [n]}, {term: tol [n]})."""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    n, x_d = len(x), x.shape[-1]
    v = x - y if residual else x
    lj = np.zeros(n)
    lj_abs = np.zeros(n)
    if logit_a:
        a = float(logit_a)
        c1 = 1.0 - 2.0 * a
        span = np.log((1 - a) / a) - np.log(a / (1 - a))
        e = a + c1 * v
        terms = np.log(c1) - np.log(e) - np.log1p(-e) - np.log(span)
        lj, lj_abs = terms.reshape(n, -1).sum(1), np.abs(terms).reshape(n, -1).sum(1)
        v = logit_preprocess(v, a)
    zy, ld, abs_s = ora.forward(np.concatenate([v, y], axis=-1), P, abs_s=True)
    z = zy[..., :x_d].reshape(n, -1)
    q = (z * z).sum(1)
    llz = -0.5 * q - 0.5 * z.shape[1] * LOG_2PI
    y_hat = zy[..., x_d:].reshape(n, -1)
    ref = {'llz': llz, 'logdet': ld, 'log_jac': lj, 'y_dev': np.abs(y_hat - y.reshape(n, -1)).sum(1),
           'log_prob': llz + ld + lj}
    tol = {'llz': RTOL * np.maximum(np.abs(llz), 0.5 * q),
           'logdet': RTOL * np.maximum(np.abs(ld), abs_s),
           'log_jac': RTOL * np.maximum(np.abs(lj), lj_abs),
           'y_dev': RTOL * y_hat.shape[1] * np.abs(zy).reshape(n, -1).max(1),
           'log_prob': RTOL * np.maximum(np.abs(llz) + np.abs(ld) + np.abs(lj), 0.5 * q + abs_s + lj_abs)}
    return ref, tol


def check_terms(out, ref, tol, what):
    worst = {}
    for name in ('log_prob', 'llz', 'logdet', 'log_jac', 'y_dev'):
        got = out[name].cpu().numpy().astype(np.float64).reshape(-1)
        assert np.isfinite(got).all(), (what, name, got)
        e = np.abs(got - ref[name])
        worst[name] = float(np.max(e / np.maximum(tol[name], 1e-300))) if tol[name].max() > 0 else float(e.max())
        print(f'{what} {name}: max abs err {e.max():.3e}, worst err/tol {worst[name]:.3f} '
              f'(|ref| <= {np.abs(ref[name]).max():.3e})')
    for name in worst:
        got = out[name].cpu().numpy().astype(np.float64).reshape(-1)
        assert np.all(np.abs(got - ref[name]) <= tol[name]), (what, name, got, ref[name], tol[name])


def _pairs(x, y):
    """the B*K expanded pairs of x [B,...], y [K,...], pair i = (i // K, i % K)"""
    B, K = len(x), len(y)
    return np.repeat(x, K, axis=0), np.tile(y, (B,) + (1,) * (y.ndim - 1))


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


CASES = [('tiny', 'plain'), ('tiny', 'logit'), ('tiny', 'residual'), ('small', 'plain'), ('small', 'logit')]


@pytest.mark.gpu
@pytest.mark.parametrize('regime', ['init', 'trained'])
@pytest.mark.parametrize('name,mode', CASES)
def test_terms_match_oracle(gpu, name, mode, regime):
    """Every term of the pairwise call, B = 3 images x K = 5 conditions, against the float64 oracle under the
    bounds of the module docstring. Measured worst err/tol: see DESIGN.md (density of given images)."""
    flow, ora, P = _setup(name, regime)
    x, y = _inputs(name, mode)
    out = flow.log_prob(torch.from_numpy(x).to(gpu), torch.from_numpy(y).to(gpu), pairwise=True, return_terms=True,
                        **MODES[mode])
    assert all(out[k].shape == (B_IMG, K_COND) for k in ('log_prob', 'llz', 'logdet', 'log_jac', 'y_dev'))
    ref, tol = log_prob_reference(ora, P, *_pairs(x, y), **MODES[mode])
    if mode != 'logit':
        assert float(out['log_jac'].abs().max()) == 0.0
    check_terms(out, ref, tol, f'{name} {mode} {regime}')


@pytest.mark.gpu
@pytest.mark.parametrize('name,mode', CASES)
def test_own_draws_match_oracle(gpu, name, mode):
    """x = the model's own draws (sample()'s 'samples' with the same logit_a / residual), each under the
    condition it was drawn for: the same oracle and bounds. With the logit map the draws are taken at temperature
    0.1: de_logitify returns the domain's edge exactly for a flow-space value above 2.3 (the fp32 logistic
    saturates; the density there is -inf by definition) and squeezes everything below -1 into a few ulp of the
    other edge, where an fp32 x no longer pins down log(e) to 1e-5; the untrained presets draw such values at
    temperature 1. Printed, not asserted: log_prob - log_jac - sample's log_prob, which carries the fp32 round
    trip and, at these untrained weights, y_hat != y (log_prob conditions on the y it is given, sample's
    log_prob belongs to the pair the inverse returned); DESIGN.md records the worst value."""
    flow, ora, P = _setup(name)
    x_d, S = PRESETS[name].x_d, K_COND
    y = torch.from_numpy(np.ascontiguousarray(_batch(name, B_IMG, 5)[..., x_d:])).to(gpu)
    drawn = flow.sample(y, S, temperature=0.1 if mode == 'logit' else 1.0, seed=3, return_stats=False,
                        return_log_prob=True, **MODES[mode])
    x = drawn['samples'].reshape((B_IMG * S,) + tuple(drawn['samples'].shape[2:])).contiguous()
    yy = y.repeat_interleave(S, dim=0).contiguous()
    out = flow.log_prob(x, yy, return_terms=True, **MODES[mode])
    assert out['log_prob'].shape == (B_IMG * S,)
    ref, tol = log_prob_reference(ora, P, x.cpu().numpy(), yy.cpu().numpy(), **MODES[mode])
    check_terms(out, ref, tol, f'{name} {mode} own draws')
    d = (out['log_prob'].double() - out['log_jac'].double() - drawn['log_prob'].reshape(-1).double()).abs()
    print(f'{name} {mode}: worst |log_prob - log_jac - sample log_prob| {float(d.max()):.3e} '
          f'(|log_prob| <= {float(out["log_prob"].abs().max()):.3e})')
    if mode == 'plain':
        # the round trip alone: the draws under the y_hat the inverse returned with them (the documented latent)
        from arl_conditional_normalizing_flows_amd.base_functions import renew_noise
        H, W, D = PRESETS[name].io_shape
        z = renew_noise(torch.empty((B_IMG, S, H, W, x_d), device=gpu), seed=3, offset=0)
        zy = torch.cat([z, y[:, None].expand(B_IMG, S, H, W, D - x_d)], dim=-1).reshape(B_IMG * S, H, W, D)
        xy_hat = flow(zy.contiguous(), -1)
        assert same_bits(xy_hat[..., :x_d].contiguous(), x)
        rt = flow.log_prob(x, xy_hat[..., x_d:].contiguous())['log_prob']
        d = (rt.double() - drawn['log_prob'].reshape(-1).double()).abs()
        print(f'{name} {mode}: under y_hat instead of y, worst |log_prob - sample log_prob| {float(d.max()):.3e}')


def _gpu_inputs(gpu, name, mode):
    x, y = _inputs(name, mode)
    return torch.from_numpy(x).to(gpu), torch.from_numpy(y).to(gpu)


ALL_KEYS = ('log_prob', 'llz', 'logdet', 'log_jac', 'y_dev', 'posterior', 'log_evidence', 'bits_per_dim')


@pytest.mark.gpu
@pytest.mark.parametrize('name,mode', CASES)
def test_pairwise_equals_paired(gpu, name, mode):
    """[B,K] of one pairwise call == the paired call on the B*K expanded pairs, bit for bit, every term; and the
    same bits from x and y at addresses that are not 16-byte aligned (the element-by-element gather)."""
    flow, ora, P = _setup(name)
    x, y = _gpu_inputs(gpu, name, mode)
    pw = flow.log_prob(x, y, pairwise=True, return_terms=True, **MODES[mode])
    xe, ye = _pairs(x.cpu().numpy(), y.cpu().numpy())
    pd = flow.log_prob(torch.from_numpy(xe).to(gpu), torch.from_numpy(ye).to(gpu), return_terms=True, **MODES[mode])
    xo = torch.empty(x.numel() + 1, device=gpu)[1:].view(x.shape).copy_(x)
    yo = torch.empty(y.numel() + 1, device=gpu)[1:].view(y.shape).copy_(y)
    assert xo.data_ptr() % 16 == 4 and yo.data_ptr() % 16 == 4 and xo.is_contiguous()
    off = flow.log_prob(xo, yo, pairwise=True, return_terms=True, **MODES[mode])
    for k in ('log_prob', 'llz', 'logdet', 'log_jac', 'y_dev', 'bits_per_dim'):
        assert torch.isfinite(pw[k]).all()
        assert same_bits(pw[k].reshape(-1), pd[k]), f'{name} {mode}: {k} differs between pairwise and paired'
        assert same_bits(pw[k], off[k]), f'{name} {mode}: {k} differs at an unaligned address'


@pytest.mark.gpu
@pytest.mark.parametrize('name,mode', CASES)
def test_no_dependence_on_chunk(gpu, name, mode):
    """chunk in {1, 4, 7, B K, 64} (chunks straddle images): every term and the posterior bit-equal; the values
    differ across the conditions of an image, so the comparison is not vacuous."""
    flow, ora, P = _setup(name)
    x, y = _gpu_inputs(gpu, name, mode)
    ref = None
    for chunk in (1, 4, 7, B_IMG * K_COND, 64):
        got = flow.log_prob(x, y, pairwise=True, chunk=chunk, return_terms=True, return_posterior=True, **MODES[mode])
        assert sorted(got) == sorted(ALL_KEYS)
        ref = got if ref is None else ref
        for k in ALL_KEYS:
            assert same_bits(got[k], ref[k]), f'{name} {mode} chunk={chunk}: {k} differs'
    assert (ref['log_prob'].max(dim=1).values > ref['log_prob'].min(dim=1).values).all()
    assert torch.isfinite(ref['log_prob']).all()


def _relaunch_all(flow, stream):
    lib = _lib.load()
    n = lib.cnf_plan_num_recorded_launches(flow._plan)
    for i in range(n):
        _lib.check(lib.cnf_plan_relaunch(flow._plan, i, stream), 'cnf_plan_relaunch')
    return n


def _launch_names(flow):
    lib = _lib.load()
    buf = C.create_string_buffer(256)
    names = []
    for i in range(lib.cnf_plan_num_recorded_launches(flow._plan)):
        _lib.check(lib.cnf_plan_recorded_launch_info(flow._plan, i, buf, 256, None, None), 'info')
        names.append(buf.value.decode())
    return names


@pytest.mark.gpu
@pytest.mark.parametrize('name,mode', [('tiny', 'residual'), ('small', 'logit')])
def test_no_dependence_on_state(gpu, name, mode):
    """The same bits after the workspace was filled with 0xFF bytes (every float a NaN), on another stream, and
    from cnf_plan_relaunch of the recorded launches into NaN-filled outputs; the recording holds, per chunk,
    k_logp_gather, the forward's launches and k_logp_finish, then k_logp_posterior."""
    flow, ora, P = _setup(name)
    x, y = _gpu_inputs(gpu, name, mode)
    kw = dict(pairwise=True, chunk=4, return_terms=True, return_posterior=True, **MODES[mode])
    ref = flow.log_prob(x, y, **kw)
    torch.cuda.synchronize()
    ref = {k: v.clone() for k, v in ref.items()}

    def check(what, got):
        torch.cuda.synchronize()
        for k in ALL_KEYS:
            assert same_bits(got[k], ref[k]), f'{name} {mode} {what}: {k} differs'

    ws = flow._ws[('log_prob', 4)]
    ws.fill_(0xFF)
    check('NaN workspace', flow.log_prob(x, y, **kw))
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = flow.log_prob(x, y, **kw)
    side.synchronize()
    check('side stream', got)
    # the recording of one call, replayed into the same (NaN-filled) outputs over a NaN-filled workspace
    out = flow.log_prob(x, y, **kw)
    names = _launch_names(flow)
    fwd = FORWARD_SCHEDULE[name]
    chunks = -(-B_IMG * K_COND // 4)
    assert names == (['k_logp_gather'] + fwd + ['k_logp_finish']) * chunks + ['k_logp_posterior']
    torch.cuda.synchronize()
    ws.fill_(0xFF)
    for k in ALL_KEYS:
        if k != 'bits_per_dim':
            out[k].fill_(float('nan'))
    assert _relaunch_all(flow, torch.cuda.current_stream().cuda_stream) == len(names)
    out['bits_per_dim'] = ref['bits_per_dim']   # (computed by torch from log_prob, not a launch)
    check('relaunch', out)


def _posterior_reference(log_prob, log_prior):
    a = log_prob.double() + (log_prior.double() if log_prior is not None else 0.0)
    return torch.log_softmax(a, dim=1).exp(), torch.logsumexp(a, dim=1), a


def check_posterior(out, log_prior, what):
    K = out['log_prob'].shape[1]
    post, lse, a = _posterior_reference(out['log_prob'], log_prior)
    ulp1 = float(np.spacing(np.float32(1.0)))
    d = (out['posterior'].double() - post).abs()
    print(f'{what}: worst posterior err {float(d.max()):.3e} (bound {4 * K * ulp1:.3e}), '
          f'largest off-peak posterior {float(post.sort(dim=1).values[:, -2].max()):.3e}')
    assert float(d.max()) <= 4 * K * ulp1
    assert float((out['posterior'].double().sum(dim=1) - 1.0).abs().max()) <= 4 * K * ulp1
    fin = torch.isfinite(a)
    big = torch.where(fin, a.abs(), torch.zeros_like(a)).max(dim=1).values.cpu().numpy()
    bound = np.spacing(big.astype(np.float32)).astype(np.float64)
    e = (out['log_evidence'].double() - lse).abs().cpu().numpy()
    assert np.all(e <= bound), (e, bound)


@pytest.mark.gpu
@pytest.mark.parametrize('name,mode', [('tiny', 'plain'), ('small', 'logit')])
def test_posterior(gpu, name, mode):
    """posterior == exp(log_softmax(log_prob + log_prior)) in float64 from the returned log_prob within 4 K fp32
    ulp of 1, rows sum to 1 within the same, log_evidence == the float64 log-sum-exp within one ulp at the
    largest |entry|; with a uniform prior, with a prior that levels the first image's row (so several classes
    carry weight) and with a class ruled out by a -inf prior, whose posterior is exactly 0."""
    flow, ora, P = _setup(name)
    x, y = _gpu_inputs(gpu, name, mode)
    uni = flow.log_prob(x, y, pairwise=True, return_posterior=True, **MODES[mode])
    assert uni['posterior'].shape == (B_IMG, K_COND) and uni['log_evidence'].shape == (B_IMG,)
    check_posterior(uni, None, f'{name} {mode} uniform')
    prior = (-uni['log_prob'][0] + torch.linspace(-1.0, 1.0, K_COND, device=gpu)).contiguous()
    lev = flow.log_prob(x, y, pairwise=True, log_prior=prior, **MODES[mode])
    assert same_bits(lev['log_prob'], uni['log_prob'])
    check_posterior(lev, prior, f'{name} {mode} levelled')
    assert float(lev['posterior'][0].min()) > 0.02
    prior[2] = float('-inf')
    out = flow.log_prob(x, y, pairwise=True, log_prior=prior, **MODES[mode])
    check_posterior(out, prior, f'{name} {mode} one class ruled out')
    assert torch.equal(out['posterior'][:, 2], torch.zeros(B_IMG, device=gpu))


@pytest.mark.gpu
def test_posterior_over_many_conditions(gpu):
    """K = 70 > 64: a row per workgroup instead of per wave; the same bounds, and an image no condition explains
    (every entry -inf) has a NaN posterior and -inf evidence while the other rows keep their bits."""
    flow, ora, P = _setup('tiny')
    K = 70
    x = _gpu_inputs(gpu, 'tiny', 'logit')[0][:2].contiguous()
    y = torch.from_numpy(np.ascontiguousarray(_batch('tiny', K, 7)[..., 1:])).to(gpu)
    prior = torch.linspace(-3.0, 3.0, K, device=gpu)
    out = flow.log_prob(x, y, pairwise=True, log_prior=prior, logit_a=LOGIT_A)
    assert out['posterior'].shape == (2, K)
    check_posterior(out, prior, 'tiny K=70')
    bad = x.clone()
    bad[1, 3, 4, 0] = 1.5   # outside de_logitify's range
    got = flow.log_prob(bad, y, pairwise=True, log_prior=prior, logit_a=LOGIT_A)
    assert torch.isneginf(got['log_prob'][1]).all() and torch.isnan(got['posterior'][1]).all()
    assert float(got['log_evidence'][1]) == float('-inf')
    for k in ('log_prob', 'posterior', 'log_evidence'):
        assert same_bits(got[k][0], out[k][0])


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['tiny', 'small'])
def test_domain_edge(gpu, name):
    """logit_a = 0.01: x exactly 0 and exactly 1 lie inside the map's domain (e = a and 1 - a) and give finite
    terms; one element pushed outside it (above, below, or NaN) gives -inf for that image's pairs and leaves the
    bits of every other pair unchanged."""
    flow, ora, P = _setup(name)
    x, y = _gpu_inputs(gpu, name, 'logit')
    x = x.clone()
    x[0, 0, 0, 0], x[0, 1, 2, 0], x[2, 5, 5, 0] = 0.0, 1.0, 1.0
    kw = dict(pairwise=True, return_terms=True, return_posterior=True, logit_a=LOGIT_A)
    ref = flow.log_prob(x, y, **kw)
    for k in ALL_KEYS:
        assert torch.isfinite(ref[k]).all(), k
    for value in (1.02, -0.02, float('nan')):
        bad = x.clone()
        bad[1, 2, 3, 0] = value
        got = flow.log_prob(bad, y, **kw)
        assert torch.isneginf(got['log_prob'][1]).all() and torch.isneginf(got['log_jac'][1]).all(), value
        assert torch.isposinf(got['bits_per_dim'][1]).all()
        assert torch.isnan(got['posterior'][1]).all() and float(got['log_evidence'][1]) == float('-inf')
        for k in ALL_KEYS:
            for b in (0, 2):
                assert same_bits(got[k][b], ref[k][b]), f'{name} x={value}: {k} of image {b} changed'


@pytest.mark.gpu
def test_python_surface(gpu):
    """Shapes, the inference of pairwise and its error, the bits_per_dim identity, the keys per switch, x and y
    of rank 3, and the workspace cached under its own key."""
    flow, ora, P = _setup('small')
    H, W, D = PRESETS['small'].io_shape
    x_d = PRESETS['small'].x_d
    x, y = _gpu_inputs(gpu, 'small', 'plain')
    out = flow.log_prob(x, y[:B_IMG])
    assert sorted(out) == ['bits_per_dim', 'log_prob'] and out['log_prob'].shape == (B_IMG,)
    assert torch.equal(out['bits_per_dim'], out['log_prob'] * (-1.0 / (H * W * x_d * np.log(2.0))))
    assert ('log_prob', B_IMG) in flow._ws
    with pytest.raises(ValueError, match='pairwise=True'):
        flow.log_prob(x, y)
    with pytest.raises(ValueError, match='one condition per image'):
        flow.log_prob(x, y, pairwise=False)
    pw = flow.log_prob(x, y, pairwise=True, return_terms=True)
    assert sorted(pw) == ['bits_per_dim', 'llz', 'log_jac', 'log_prob', 'logdet', 'y_dev']
    assert all(v.shape == (B_IMG, K_COND) and v.dtype == torch.float32 for v in pw.values())
    assert same_bits(pw['log_prob'][:, :B_IMG].diagonal(), out['log_prob'])
    # the terms add up to log_prob: three fp32 roundings (llz, log_jac, the sum), each at most half an ulp at
    # M = |llz| + |logdet| + |log_jac|
    s = pw['llz'].double() + pw['logdet'].double() + pw['log_jac'].double()
    M = (pw['llz'].abs() + pw['logdet'].abs() + pw['log_jac'].abs()).cpu().numpy()
    assert torch.all((pw['log_prob'].double() - s).abs() <= torch.from_numpy(1.5 * np.spacing(M).astype(np.float64)).to(gpu))
    one = flow.log_prob(x[1], y[2])   # rank 3: one image, one condition
    assert one['log_prob'].shape == (1,) and same_bits(one['log_prob'], pw['log_prob'][1, 2:3])
    row = flow.log_prob(x[1], y, pairwise=True, return_posterior=True)
    assert row['posterior'].shape == (1, K_COND) and same_bits(row['log_prob'][0], pw['log_prob'][1])
    col = flow.log_prob(x, y[2], pairwise=True)
    assert col['log_prob'].shape == (B_IMG, 1) and same_bits(col['log_prob'][:, 0], pw['log_prob'][:, 2])
    with pytest.raises(AssertionError, match='pairwise'):
        flow.log_prob(x, y[:B_IMG], return_posterior=True)
    with pytest.raises(ValueError, match='log_prior'):
        flow.log_prob(x, y, pairwise=True, log_prior=torch.zeros(K_COND + 1, device=gpu))
    with pytest.raises(AssertionError, match='residual'):
        flow.log_prob(x, y, pairwise=True, residual=True)   # small: D - x_d != x_d
    with pytest.raises(ValueError, match='x has shape'):
        flow.log_prob(y, y)
