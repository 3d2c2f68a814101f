"""The flow kernels at values OracleCFlow.init_params never produces.

Every other GPU test draws its weights from init_params (Orthogonal(gain=0.1) kernels, small
perturbations of bias / gamma / beta / w): the flow before its first training step, near the identity,
every pre-tanh activation A small. cpl_tanh (csrc/cnf_device.h) has a Taylor branch below |A| = 0.25
and 1 - 2 rcp(exp(2|A|) + 1) above; with init_params the upper branch, which a trained model runs
almost everywhere, is taken by 0 % (tiny) / 0.4 % (small) of the elements (test_census). REGIMES holds
weight transformations, each a pure function P -> P of init_params(seed), that reach the rest of the
value-dependent machinery: the saturating tanh, exp at |s| > 0.3 and the inverse's 1 / exp(s), LN
statistics whose mean is ~300 times their spread or whose variance is 0, LN gamma / beta far from
(1, 0), a negative tanh_scale.w, the bf16x6 split on operands several times larger.

CPU part: the census (the coverage claim), every regime finite and invertible in float64, and the
float64 torch-CPU restatement equal to the numpy oracle off the default weights too.

GPU part.
* The law sweep: conv_out.kernel = 0 on both nets makes s = w tanh(bias_A[c]) and t = bias_b[c] known
  answers; a grid of pre-tanh values from 0 to the exp overflow is spread over the layers' biases and
  every coupling layer is compared with the float64 oracle element by element under bounds derived from
  the error claims written in cnf_device.h.
* Regime parity: forward, per-image log-det, inverse and NLL against float64. In these regimes the
  project's 1e-5 bounds are out of reach of any fp32 implementation (fp32 torch-CPU, trained-like
  weights, inverse: 4e-3), so each error is bounded by max(the existing bound, K_FP32 x the error of
  the fp32 torch-CPU restatement on the identical inputs) per image, as test_train._tol does for
  gradients. The bounds themselves are imported from test_gpu_parity / test_train, not restated.
* The bit-for-bit contracts (layerwise == fused, batch independence) and the training gradient on
  saturated weights.

Weights are rounded to fp32 before either side sees them, so the comparison is of arithmetic alone.

When the file was added the lnoffset / lnconst rows failed by two to three orders of magnitude: the shift
of k_net_lds's LN partial sums in the residual epilogue, the merges of partial means and the
fma(t, rstd, -mean * rstd) normalisation all erred relative to the mean instead of the spread (fixed in
csrc/cnf_device.h, cnf_netlds.hip, cnf_stream.hip, cnf_kernels.hip)."""
import functools
import os

import numpy as np
import pytest
import torch

from arl_conditional_normalizing_flows_amd.config import PRESETS
from oracle import cflow_np as O
from oracle.cflow_np import OracleCFlow, synthetic_class_batch
from oracle.cflow_torch_cpu import TorchCPUFlow

from test_gpu_parity import RTOL, ld_tol

# e_gpu <= max(existing bound, K_FP32 * e_32): the smallest power of two that is at least twice the worst
# e_gpu / e_32 measured on the MI355X over every row whose error exceeds the existing bound (3.26, tiny
# negw inverse; DESIGN.md section 3, "Values off the initialisation"), and the cap: the GPU rounds along
# another path than a plain fp32 graph, it has no licence to be an order of magnitude worse
K_FP32 = 8.0

WEIGHT_SEED = 2   # the census's weights and batch
BATCH_SEED = 4


# ---------------------------------------------------------------------------------------------
# regimes
# ---------------------------------------------------------------------------------------------

def _map(P, fn):
    """fn(name, value) -> new value or None (unchanged); never modifies P"""
    out = {}
    for k, v in P.items():
        r = fn(k, np.asarray(v, np.float64))
        out[k] = np.asarray(v if r is None else r, np.float64)
    return out


def _kernels_times(f, only=''):
    return lambda P: _map(P, lambda k, v: v * f if k.endswith('.kernel') and only in k else None)


def _trained(P):
    """every parameter kind as after some epochs: kernels x3 (x8 on conv_out), bias ~ N(0, 0.3),
    gamma = 1 + N(0, 0.5), beta ~ N(0, 0.5), tanh_scale.w = 2"""
    rng = np.random.default_rng(9)

    def fn(k, v):
        if k.endswith('.kernel'):
            return v * (8.0 if '.conv_out.' in k else 3.0)
        if k.endswith('.bias'):
            return rng.normal(0, 0.3, v.shape)
        if k.endswith('.gamma'):
            return 1.0 + rng.normal(0, 0.5, v.shape)
        if k.endswith('.beta'):
            return rng.normal(0, 0.5, v.shape)
        if k.endswith('.w'):
            return np.asarray(2.0)
    return _map(P, fn)


def _negw(P):
    """out8 with tanh_scale.w = -1.5 on odd coupling indices, +3 on even ones"""
    def fn(k, v):
        if k.endswith('.tanh_scale.w'):
            return np.asarray(-1.5 if int(k.split('.')[0][1:]) % 2 else 3.0)
    return _map(REGIMES['out8'](P), fn)


def _lnoffset(P):
    """conv_in.bias += 30 on both nets: the first LN of every net sees mean ~ 300 x spread"""
    return _map(P, lambda k, v: v + 30.0 if k.endswith('.conv_in.bias') else None)


def _lnconst(bias):
    """net b: conv_in.kernel = 0, conv_in.bias = bias: LN1 of its first residual block sees an exactly
    constant image (variance 0)"""
    def fn(k, v):
        if '.b.conv_in.kernel' in k:
            return np.zeros_like(v)
        if '.b.conv_in.bias' in k:
            return np.full_like(v, bias)
    return lambda P: _map(P, fn)


REGIMES = {
    'default': lambda P: _map(P, lambda k, v: None),
    'gain0.5': _kernels_times(5.0),
    'out8': _kernels_times(8.0, '.A.conv_out.'),
    'out30': _kernels_times(30.0, '.A.conv_out.'),
    'trained': _trained,
    'negw': _negw,
    'lnoffset': _lnoffset,
    'lnconst3': _lnconst(3.0),
    'lnconst1000': _lnconst(1000.0),
}
OFF_INIT = [r for r in REGIMES if r != 'default']

# census floors: share of |A| >= 0.25, share of |A| >= 2 (over every coupling layer, tiny and small)
FLOORS = {'gain0.5': (0.5, None), 'out8': (0.6, None), 'out30': (0.85, 0.3), 'trained': (0.7, 0.02)}


def _f32(P):
    """the weights as the device holds them (fp32), kept in float64 arrays"""
    return {k: np.asarray(np.asarray(v, np.float32), np.float64) for k, v in P.items()}


def regime_params(ora, regime, seed=WEIGHT_SEED):
    return _f32(REGIMES[regime](ora.init_params(seed)))


def _kw(name, group_mode='reference', **extra):
    return dict(PRESETS[name].kwargs(), group_mode=group_mode, **extra)


def _batch(name, B, seed=BATCH_SEED):
    cfg = PRESETS[name]
    H, W, _ = cfg.io_shape
    return synthetic_class_batch(B, H, W, cfg.x_d, seed=seed)


def pre_tanh(ora, xy, P):
    """|A| of every coupling layer of the float64 oracle's forward (the input of np.tanh in st_net): the
    oracle's conv2d_same is wrapped for the call and the outputs of net A's conv_out are recorded.
    Returns (list of |A| per coupling layer, zy)."""
    P = ora._cast(P, np.float64)
    mine = {id(v) for k, v in P.items() if k.endswith('.A.conv_out.kernel')}
    rec = []
    orig = O.conv2d_same

    def recording(x, kernel, bias, dilation=1):
        y = orig(x, kernel, bias, dilation)
        if id(kernel) in mine:
            rec.append(np.abs(y).ravel())
        return y
    O.conv2d_same = recording
    try:
        zy, _ = ora.forward(xy, P)
    finally:
        O.conv2d_same = orig
    assert len(rec) == len(ora.coupling_specs)
    return rec, zy


# ---------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _census(name, regime):
    ora = OracleCFlow(**_kw(name))
    xy = _batch(name, 3)
    P = regime_params(ora, regime)
    with np.errstate(over='ignore'):
        rec, zy = pre_tanh(ora, xy, P)
        x_back = ora.inverse(zy, P)
    a = np.concatenate(rec)
    rt = float(np.max(np.abs(x_back - xy)) / np.max(np.abs(xy)))
    return float(np.mean(a >= 0.25)), float(np.mean(a >= 2.0)), float(a.max()), bool(np.isfinite(zy).all()), rt


@pytest.mark.parametrize('name', ['tiny', 'small'])
def test_census(name):
    """Why this file exists: with init_params the upper branch of cpl_tanh is all but unreached, and the
    saturating regimes reach it on most elements. The floors are conditions on the regime functions
    (replace them by the identity and this fails), not measurements."""
    lo, hi, amax, _, _ = _census(name, 'default')
    print(f'{name} default: share |A| >= 0.25 {lo:.4f}, >= 2 {hi:.4f}, max |A| {amax:.2f}')
    assert lo < 0.01 and hi == 0.0
    for regime, (f_lo, f_hi) in FLOORS.items():
        lo, hi, amax, _, _ = _census(name, regime)
        print(f'{name} {regime}: share |A| >= 0.25 {lo:.4f}, >= 2 {hi:.4f}, max |A| {amax:.2f}')
        assert lo >= f_lo, (regime, lo)
        assert f_hi is None or hi >= f_hi, (regime, hi)


@pytest.mark.parametrize('regime', OFF_INIT)
@pytest.mark.parametrize('name', ['tiny', 'small'])
def test_regime_is_finite_and_invertible_in_float64(name, regime):
    _, _, _, finite, rt = _census(name, regime)
    assert finite
    assert rt <= 1e-10, rt


def test_regimes_are_pure_and_deterministic():
    ora = OracleCFlow(**_kw('tiny'))
    P0 = ora.init_params(WEIGHT_SEED)
    keep = {k: np.array(v, copy=True) for k, v in P0.items()}
    for regime, fn in REGIMES.items():
        a, b = fn(P0), fn(P0)
        assert all(np.array_equal(a[k], b[k]) for k in P0), regime
        assert all(np.array_equal(P0[k], keep[k]) for k in P0), regime
        changed = any(not np.array_equal(a[k], P0[k]) for k in P0)
        assert changed == (regime != 'default'), regime
    # lnconst: LN1 of net b's first residual block sees a constant image (conv_in output == bias everywhere)
    P = regime_params(ora, 'lnconst1000')
    c = ora.coupling_specs[0]
    y = O.conv2d_same(np.random.default_rng(0).standard_normal((2, c.hc, c.wc, c.dc1)),
                      P['c0.b.conv_in.kernel'], P['c0.b.conv_in.bias'])
    assert np.all(y == 1000.0)


@pytest.mark.parametrize('regime', ['trained', 'lnoffset'])
def test_torch_cpu_float64_is_the_numpy_oracle_off_init(regime):
    """test_oracle.test_torch_cpu_float64_is_the_numpy_oracle on weights off the initialisation: the fp32
    yardstick of the GPU tests below is the same graph as the float64 oracle."""
    kw = _kw('tiny')
    ora = OracleCFlow(**kw)
    P = regime_params(ora, regime)
    xy = _batch('tiny', 3)
    zr, lr, ar = ora.forward(xy, P, abs_s=True)
    xr = ora.inverse(zr.astype(np.float32), P)
    zt, lt, at, xt = _torch_run(kw, P, xy, zr.astype(np.float32), torch.float64)
    for got, ref in ((zt, zr), (lt, lr), (at, ar), (xt, xr)):
        assert np.max(np.abs(got - ref)) <= 1e-10 * max(1.0, np.max(np.abs(ref)))


# ---------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------

def _torch_run(kw, P, xy, z_in, dtype):
    """TorchCPUFlow in dtype: (zy, per-image log-det, per-image sum|s|, inverse of z_in) as float64 numpy"""
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    t = TorchCPUFlow(**kw)
    T = {k: torch.from_numpy(np.asarray(v, np.float64)).to(dtype) for k, v in P.items()}
    with torch.no_grad():
        zy, st = t.forward(torch.from_numpy(np.asarray(xy, np.float64)).to(dtype), T, per_image=True)
        x = t.inverse(torch.from_numpy(np.asarray(z_in, np.float64)).to(dtype), T)
    return zy.double().numpy(), st[0].double().numpy(), st[1].double().numpy(), x.double().numpy()


class Ref:
    pass


@functools.lru_cache(maxsize=None)
def _refs(name, B, regime, group_mode='reference'):
    """float64 and fp32 CPU results of a (flow, regime), computed once and left unchanged. The inverse's
    input is the float64 zy cast to fp32: the GPU, the fp32 reference and the float64 inverse all get
    that tensor. float64: the numpy oracle (tiny, small), its torch restatement (cfg2)."""
    r = Ref()
    r.kw = _kw(name, group_mode)
    r.ora = OracleCFlow(**r.kw)
    r.P = regime_params(r.ora, regime)
    r.xy = _batch(name, B)
    if name == 'cfg2':
        r.zy, r.ld, r.abs_s, _ = _torch_run(r.kw, r.P, r.xy, r.xy, torch.float64)
        r.z_in = r.zy.astype(np.float32)
        r.x = _torch_run(r.kw, r.P, r.xy, r.z_in, torch.float64)[3]
    else:
        r.zy, r.ld, r.abs_s = r.ora.forward(r.xy, r.P, abs_s=True)
        r.z_in = r.zy.astype(np.float32)
        r.x = r.ora.inverse(r.z_in, r.P)
    r.zy32, r.ld32, _, r.x32 = _torch_run(r.kw, r.P, r.xy, r.z_in, torch.float32)
    # the NLL 4-tuple: float64 from the float64 forward, fp32 as the fp32 graph computes it
    llz, lly, _ = r.ora.nll_terms(r.xy.astype(np.float64), r.zy, r.ld)
    r.nll = [-((llz + lly).mean() + r.ld.mean()), -llz.mean(), -lly.mean(), -r.ld.mean()]
    with torch.no_grad():
        r.nll32 = [float(t) for t in TorchCPUFlow(**r.kw).log_loss(
            torch.tensor(r.xy), {k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in r.P.items()})]
    for a in (r.xy, r.zy, r.ld, r.abs_s, r.z_in, r.x, r.zy32, r.ld32, r.x32):
        a.setflags(write=False)
    return r


def _err_img(a, ref):
    """test_gpu_parity._err per image: max|a - ref| / max|ref| over each image"""
    a = np.asarray(a, np.float64).reshape(len(ref), -1)
    b = np.asarray(ref, np.float64).reshape(len(ref), -1)
    return np.max(np.abs(a - b), axis=1) / np.maximum(np.max(np.abs(b), axis=1), 1e-30)


def _flow(kw, P, gpu, options=None):
    from arl_conditional_normalizing_flows_amd.make_model import cFlow
    flow = cFlow(**kw, device=gpu, debug_options=options)
    flow.set_weights(P)
    return flow


def _ratio(e_gpu, e_32):
    """worst e_gpu / e_32 over the images whose error exceeds the existing bound (elsewhere the existing
    bound decides and the ratio is of two rounding noises)"""
    m = e_gpu > RTOL
    return float(np.max(e_gpu[m] / np.maximum(e_32[m], 1e-30))) if m.any() else 0.0


# ---------------------------------------------------------------------------------------------
# GPU: the law sweep
# ---------------------------------------------------------------------------------------------

# pre-tanh values: both branches of cpl_tanh and their seam, tanh rounding to 1 (8.5, 9.1), exp(2|x|)
# overflowing to inf (44.4, 100)
GRID = [0.0] + [s * v for v in (1e-20, 1e-3, 0.2499, 0.25, 0.2501, 0.5, 1.0, 2.0, 4.0, 8.5, 9.1, 20.0, 44.4, 100.0)
                for s in (1.0, -1.0)]
LAW_W = (1.0, 3.0, -0.5)
LAW_T = (0.0, 0.7, -0.7)
LAW_VARIANTS = 8   # tiny's channel-mask layers hold 4 bias entries: 8 variants walk the 29 grid values


def law_params(ora, variant):
    """Both nets' conv_out.kernel = 0: s = w tanh(bias_A[c]), t = bias_b[c] whatever the input. The grid
    is laid consecutively over the checkerboard layers' bias entries and, separately, over the
    channel-mask layers', each variant starting where the previous one ended. Returns (P, {kind: set of
    grid indices placed})."""
    P = dict(ora.init_params(WEIGHT_SEED))
    specs = ora.coupling_specs
    kind = lambda c: 'cb' if c.mask in (0, 1) else 'ch'
    per_run = {k: sum(c.dc2 for c in specs if kind(c) == k) for k in ('cb', 'ch')}
    at = {k: variant * per_run[k] for k in per_run}
    placed = {'cb': set(), 'ch': set()}
    for li, c in enumerate(specs):
        p, k = f'c{c.index}', kind(c)
        idx = (at[k] + np.arange(c.dc2)) % len(GRID)
        at[k] += c.dc2
        placed[k].update(idx.tolist())
        for net in 'Ab':
            P[f'{p}.{net}.conv_out.kernel'] = np.zeros_like(P[f'{p}.{net}.conv_out.kernel'])
        P[f'{p}.A.conv_out.bias'] = np.asarray(GRID)[idx]
        P[f'{p}.b.conv_out.bias'] = np.asarray(LAW_T)[(np.arange(c.dc2) + li + variant) % 3]
        P[f'{p}.A.tanh_scale.w'] = np.asarray(LAW_W[(li + variant) % 3])
    return _f32(P), placed


@pytest.mark.parametrize('name', ['tiny', 'small'])
def test_law_grid_reaches_both_mask_kinds(name):
    ora = OracleCFlow(**_kw(name))
    seen = {'cb': set(), 'ch': set()}
    ws = set()
    for variant in range(LAW_VARIANTS):
        P, placed = law_params(ora, variant)
        for k in seen:
            seen[k] |= placed[k]
        ws |= {(c.mask in (0, 1), float(P[f'c{c.index}.A.tanh_scale.w'])) for c in ora.coupling_specs}
        # known answers: s and t do not depend on the input
        c = ora.coupling_specs[-1]
        for seed in (0, 1):
            u = np.random.default_rng(seed).standard_normal((1, c.hc, c.wc, c.dc1))
            s = O.st_net(u, c, P, 'A')
            assert np.array_equal(s[0, 0, 0], P[f'c{c.index}.A.tanh_scale.w'] * np.tanh(P[f'c{c.index}.A.conv_out.bias']))
            assert np.array_equal(O.st_net(u, c, P, 'b')[0, -1, -1], P[f'c{c.index}.b.conv_out.bias'])
    full = set(range(len(GRID)))
    assert seen['cb'] == full and seen['ch'] == full
    assert ws == {(cb, w) for cb in (True, False) for w in LAW_W}


# the claims of cnf_device.h: cpl_tanh < 1e-6 relative, so s = w tanh(A) carries 1e-6 |s| (+ the product's
# rounding) and exp(s) that relative error; cpl_exp is the hardware exp2 of s * log2(e): 1 ulp of the
# result plus the rounding of the fp32 product, 2^-24 |s| log2(e) ln 2 relative. With the fma's (forward)
# or the subtraction's and product's (inverse) own roundings:
#   |dv| <= (1.2e-6 |s| + 3e-7) |e^{+-s} (x -+ t)| + 2e-7 |t|
LAW_REL_S, LAW_REL_0, LAW_ABS_T = 1.2e-6, 3e-7, 2e-7
LAW_LD = 2e-6   # per-image log-det: |d| <= 2e-6 sum|s| (1e-6 of tanh, the product, the fp32 sum)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', range(LAW_VARIANTS))
@pytest.mark.parametrize('name', ['tiny', 'small'])
def test_law_sweep(gpu, name, variant):
    kw = _kw(name)
    ora = OracleCFlow(**kw)
    P, _ = law_params(ora, variant)
    flow = _flow(kw, P, gpu)
    streamed = _flow(kw, P, gpu, {'NETLDS': 0})
    B = 3
    rng = np.random.default_rng(100 + variant)
    worst = dict(fwd=0.0, inv=0.0, ld=0.0)
    layers = [L for L in flow.layers_list if hasattr(L, 'coupling_index')]
    layers_s = [L for L in streamed.layers_list if hasattr(L, 'coupling_index')]
    for L, Ls, c in zip(layers, layers_s, ora.coupling_specs):
        p = f'c{c.index}'
        u = rng.standard_normal((B, c.H, c.W, c.D)).astype(np.float32)
        u64 = u.astype(np.float64)
        s = np.broadcast_to(P[f'{p}.A.tanh_scale.w'] * np.tanh(P[f'{p}.A.conv_out.bias']), (B, c.hc, c.wc, c.dc2))
        t = np.broadcast_to(P[f'{p}.b.conv_out.bias'], s.shape)
        x2 = O.mask_compress(u64, c.mask_c)
        ut = torch.from_numpy(u).to(gpu)
        cond = O.mask_uncompressed(np.ones_like(u64), c.mask) == 1
        # forward
        v_ref, ld_ref, abs_s = O.coupling_forward(u64, c, P, with_abs=True)
        v, ld, _ = L.forward_and_Jacobian(ut, torch.zeros(B, device=gpu), None)
        v_s, ld_s, _ = Ls.forward_and_Jacobian(ut, torch.zeros(B, device=gpu), None)
        assert torch.equal(v, v_s) and torch.equal(ld, ld_s), p
        v = v.cpu().numpy()
        bound = O.decompress((LAW_REL_S * np.abs(s) + LAW_REL_0) * np.abs(np.exp(s) * x2) + LAW_ABS_T * np.abs(t),
                             c.mask_c, u.shape)
        assert np.array_equal(v[cond], u[cond]), p        # the conditioning half passes through bit for bit
        err = np.abs(v.astype(np.float64) - v_ref)
        worst['fwd'] = max(worst['fwd'], float(np.max(err[~cond] / bound[~cond])))
        assert np.all(err[~cond] <= bound[~cond]), (p, 'forward', float(np.max(err[~cond] / bound[~cond])))
        e_ld = np.abs(ld.cpu().numpy().astype(np.float64) - ld_ref)
        worst['ld'] = max(worst['ld'], float(np.max(e_ld / np.maximum(LAW_LD * abs_s, 1e-300))))
        assert np.all(e_ld <= LAW_LD * abs_s), (p, 'log-det', e_ld, abs_s)
        # inverse
        x_ref = O.coupling_backward(u64, c, P)
        x, _ = L.backward(ut, None)
        x_s, _ = Ls.backward(ut, None)
        assert torch.equal(x, x_s), p
        x = x.cpu().numpy()
        bound = O.decompress((LAW_REL_S * np.abs(s) + LAW_REL_0) * np.abs(np.exp(-s) * (x2 - t)) + LAW_ABS_T * np.abs(t),
                             c.mask_c, u.shape)
        assert np.array_equal(x[cond], u[cond]), p
        err = np.abs(x.astype(np.float64) - x_ref)
        worst['inv'] = max(worst['inv'], float(np.max(err[~cond] / bound[~cond])))
        assert np.all(err[~cond] <= bound[~cond]), (p, 'inverse', float(np.max(err[~cond] / bound[~cond])))
    print(f'law sweep {name} variant {variant}: worst error / bound forward {worst["fwd"]:.3f} '
          f'inverse {worst["inv"]:.3f} log-det {worst["ld"]:.3f}')
    # the fused schedules (deferred law in k_net_lds / k_map2, the log-det reduction) against the per-layer
    # API, and the streamed path against the default one: bit for bit
    H, W, D = PRESETS[name].io_shape
    xy = rng.standard_normal((B, H, W, D)).astype(np.float32)
    x = torch.from_numpy(xy).to(gpu)
    zy, ld = flow(x, 1, per_image_logdet=True)
    zy_l, ld_l = flow(x, 1, per_image_logdet=True, layerwise=True)
    zy_s, ld_s = streamed(x, 1, per_image_logdet=True)
    xi, xi_l, xi_s = flow(zy, -1), flow(zy, -1, layerwise=True), streamed(zy, -1)
    torch.cuda.synchronize()
    assert torch.isfinite(zy).all() and torch.isfinite(xi).all() and torch.isfinite(ld).all()
    assert torch.equal(zy, zy_l) and torch.equal(zy, zy_s)
    assert torch.equal(xi, xi_l) and torch.equal(xi, xi_s)
    # s does not depend on the input, so the oracle's log-det of any batch is the known answer
    _, ld_ref, abs_s = ora.forward(xy, P, abs_s=True)
    for got in (ld, ld_l, ld_s):
        assert np.all(np.abs(got.cpu().numpy().astype(np.float64) - ld_ref) <= LAW_LD * abs_s)


# ---------------------------------------------------------------------------------------------
# GPU: regime parity
# ---------------------------------------------------------------------------------------------

# (preset, B, group mode, debug options)
FLOWS = {'tiny': ('tiny', 3, 'reference', None), 'small': ('small', 3, 'reference', None),
         'small_streamed': ('small', 3, 'reference', {'NETLDS': 0}),
         'small_intended': ('small', 3, 'intended', None),
         'cfg2': ('cfg2', 2, 'reference', None), 'cfg2_streamed': ('cfg2', 2, 'reference', {'NETLDS': 0})}
# The per-image log-det bound 1e-5 max(|ref|, sum|s|) is kept as it is in every regime but this one. With
# conv_in's output at 1000 the residual stream of net b is 1000 + O(0.1) in every later LayerNorm, and an
# fp32 tensor holds it to 2^-24 * 1000 = 6e-5, 6e-4 of its spread: the fp32 torch-CPU graph itself ends at
# 1.01 (tiny), 1.66 (small), 1.67 (cfg2) of the bound, the GPU at 1.05, 0.40, 1.32 (1.23 streamed). There the
# bound takes the max(existing, K_FP32 e_32) form of zy and the inverse. lnoffset, for which that form was
# held in reserve, does not need it (GPU 0.25 .. 0.35 of the bound, the fp32 graph 0.44 .. 0.76).
LOGDET_FP32_FORM = ('lnconst1000',)

PARITY = ([(f, r) for r in OFF_INIT for f in ('tiny', 'small', 'cfg2', 'cfg2_streamed')] +
          [('small_intended', 'trained')])


@pytest.mark.gpu
@pytest.mark.parametrize('flow_name,regime', PARITY)
def test_forward_logdet_inverse_match_oracle(gpu, flow_name, regime):
    name, B, gm, options = FLOWS[flow_name]
    r = _refs(name, B, regime, gm)
    flow = _flow(r.kw, r.P, gpu, options)
    zy, ld = flow(torch.tensor(r.xy).to(gpu), 1, per_image_logdet=True)
    x = flow(torch.tensor(r.z_in).to(gpu), -1)
    torch.cuda.synchronize()
    assert torch.isfinite(zy).all() and torch.isfinite(ld).all() and torch.isfinite(x).all()
    what = f'{flow_name} {regime}'
    ok = True
    for label, got, got32, ref in (('zy', zy, r.zy32, r.zy), ('inverse', x, r.x32, r.x)):
        e_gpu, e_32 = _err_img(got.cpu().numpy(), ref), _err_img(got32, ref)
        bound = np.maximum(RTOL, K_FP32 * e_32)
        print(f'{what} {label}: e_gpu {e_gpu.max():.3e} e_32 {e_32.max():.3e} worst e_gpu/bound '
              f'{np.max(e_gpu / bound):.3f} worst e_gpu/e_32 above {RTOL:g}: {_ratio(e_gpu, e_32):.2f}')
        ok = ok and bool(np.all(e_gpu <= bound))
    # the log-det keeps its bound as it is (LOGDET_FP32_FORM: the one regime where the fp32 graph misses it)
    e = np.abs(ld.cpu().numpy().astype(np.float64) - r.ld)
    e32 = np.abs(r.ld32 - r.ld)
    tol = ld_tol(r.ld, r.abs_s)
    print(f'{what} logdet: worst err/tol {np.max(e / tol):.3f} (fp32 reference {np.max(e32 / tol):.3f})')
    if regime in LOGDET_FP32_FORM:
        tol = np.maximum(tol, K_FP32 * e32)
    assert ok
    assert np.all(e <= tol), (e, tol)


@pytest.mark.gpu
@pytest.mark.parametrize('regime', ['trained', 'out30'])
@pytest.mark.parametrize('flow_name', ['tiny', 'small', 'cfg2', 'cfg2_streamed'])
def test_nll_matches_oracle(gpu, flow_name, regime):
    name, B, gm, options = FLOWS[flow_name]
    r = _refs(name, B, regime, gm)
    got = [t.item() for t in _flow(r.kw, r.P, gpu, options).log_loss(torch.tensor(r.xy).to(gpu))]
    print(f'{flow_name} {regime} nll ref {r.nll} fp32 {r.nll32} got {got}')
    for ref, g32, g in zip(r.nll, r.nll32, got):
        assert np.isfinite(g)
        # the bound of test_gpu_parity.test_nll_matches_oracle, or K_FP32 x the fp32 graph's own error
        bound = max(RTOL * max(abs(ref), r.abs_s.mean()), K_FP32 * abs(g32 - ref))
        print(f'  |err| {abs(g - ref):.3e} bound {bound:.3e} fp32 err {abs(g32 - ref):.3e}')
        assert abs(g - ref) <= bound


@pytest.mark.gpu
@pytest.mark.parametrize('regime', ['trained', 'out30'])
@pytest.mark.parametrize('flow_name', ['small', 'small_streamed', 'cfg2', 'cfg2_streamed'])
def test_bitwise_contracts_do_not_depend_on_the_values(gpu, flow_name, regime):
    """test_gpu_parity.test_layerwise_equals_fused and the batch independence of
    test_shape_sweep.test_batch_independence (7 images against batches of 3) on saturated weights."""
    name, B, gm, options = FLOWS[flow_name]
    kw = _kw(name, gm)
    P = regime_params(OracleCFlow(**kw), regime)
    flow = _flow(kw, P, gpu, options)
    x = torch.from_numpy(_batch(name, 7, seed=5)).to(gpu)
    zy, ld = flow(x, 1, per_image_logdet=True)
    xi = flow(zy, -1)
    assert torch.isfinite(zy).all() and torch.isfinite(ld).all() and torch.isfinite(xi).all()
    zy2, ld2 = flow(x[:3], 1, per_image_logdet=True, layerwise=True)
    xi2 = flow(zy[:3], -1, layerwise=True)
    assert torch.equal(zy2, zy[:3])
    assert torch.allclose(ld2, ld[:3], rtol=1e-6, atol=1e-5)
    assert torch.equal(xi2, xi[:3])
    for s in range(0, 7, 3):
        zs, ls = flow(x[s:s + 3], 1, per_image_logdet=True)
        xs = flow(zy[s:s + 3], -1)
        assert torch.equal(zs, zy[s:s + 3]), (s, (zs - zy[s:s + 3]).abs().max().item())
        assert torch.equal(ls, ld[s:s + 3]), (s, (ls - ld[s:s + 3]).abs().max().item())
        assert torch.equal(xs, xi[s:s + 3]), (s, (xs - xi[s:s + 3]).abs().max().item())


# ---------------------------------------------------------------------------------------------
# GPU: gradients on saturated weights
# ---------------------------------------------------------------------------------------------

# out30 is deliberately absent: at |A| ~ 10 the derivative 1 - tanh^2 is below fp32 resolution in every
# implementation
GRAD_CASES = [('small', 3, 'gain0.5', {}, None), ('small', 3, 'out8', {}, None), ('small', 3, 'trained', {}, None),
              ('small', 3, 'lnoffset', {}, None),
              ('cfg2', 2, 'out8', {}, None), ('cfg2', 2, 'out8', {}, {'LDS_BWD': 0}),
              ('tiny', 3, 'out8', {'LAYER_NORM': False}, None)]


@functools.lru_cache(maxsize=None)
def _grad_refs(name, B, regime, ln):
    """float64 and fp32 autograd on the regime's weights (test_train's seeds: weights 5, batch 6)"""
    from test_train import oracle_grads
    kw = _kw(name, LAYER_NORM=ln)
    P = regime_params(OracleCFlow(**kw), regime, seed=5)
    xy = _batch(name, B, seed=6)
    G_ref, terms_ref = oracle_grads(kw, P, xy)
    G32, _ = oracle_grads(kw, P, xy, torch.float32)
    return kw, P, xy, (G_ref, terms_ref, G32)


@pytest.mark.gpu
@pytest.mark.parametrize('name,B,regime,extra,options', GRAD_CASES)
def test_gradients_match_oracle(gpu, name, B, regime, extra, options):
    """test_train's bar per parameter tensor (relative to fp32 autograd's own error), no perturbation term."""
    from test_train import check_gradients
    kw, P, xy, refs = _grad_refs(name, B, regime, extra.get('LAYER_NORM', True))
    check_gradients(gpu, kw, xy, options, f'{name} {regime} {extra or ""} {options or ""}', None, refs, params=P)
