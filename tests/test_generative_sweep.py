"""The generative direction off the presets: cnf_flow_inverse_logdet / cnf_coupling_inverse_logdet, cnf_flow_sample
and cnf_flow_sample_logp (include/cnf.h) on the shape sweep's rows and on weights away from initialisation.

tests/test_inverse_logdet.py and tests/test_sampling.py run on presets (tiny, small, cfg2, twice xd1of4 /
odd_d5). The kernels that write the inverse's log-det slots index them by np = max over couplings of
min(16, ceil(hc wc / 64)): k_coupling (one slot per blockIdx.x of np blocks), the tail of k_net_lds (two slots
when np >= 2, zeros from slot 2), its comp path (slot 0, zeros from 1) and the boundary k_map2. The presets and
the sweep give np in {1, 3, 4, 16}; the row 'np2' below adds np == 2, the edge of the tail's split. The
sampling kernels (csrc/cnf_sample.hip) fold the draws of a condition in batches of FOLD_BATCH = 64 over
workgroups of FOLD_E = 32 elements and sum an image per wave: more than 64 draws of a condition in one chunk,
HW x_d % 32 != 0 and images of fewer than 64 elements are reached here and nowhere else.

Rows: test_shape_sweep.SWEEP plus 'np2'. Weights OracleCFlow.init_params(0) (through the regimes of
tests/test_value_regimes.py where named), inputs standard normal. Every helper and bound is imported from the
file that owns it; the float64 / fp32 CPU references are computed once per (row, regime).

CPU part (against the cross-compiled library): the coverage claims above, the direction -2 schedule of every
case, and that every (row, regime) the GPU part uses is finite and invertible in float64.

GPU part: see the section comments; measured figures in DESIGN.md (inverse log-det, "Values off the
initialisation", sampling)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from arl_conditional_normalizing_flows_amd import _lib
from arl_conditional_normalizing_flows_amd.config import PRESETS
from oracle import cflow_np as O
from oracle import transforms_np
from oracle.cflow_np import OracleCFlow

from test_capi import _plan, schedule_of_plan
from test_gpu_parity import RTOL, _err, check_logdet, ld_tol
from test_inverse_logdet import _composed_kw, _zy_kw, log_prob_oracle, same_bits
from test_sampling import _check_stats
from test_shape_sweep import _OPTS, _RECT, ROWS, SWEEP, _flow, _kw, _opt_str, _oracle, _row
from test_value_regimes import K_FP32, LAW_LD, LAW_VARIANTS, _err_img, _torch_run, law_params, regime_params

# np == 2 (8x16 checkerboard layers: 64 compressed pixels are one slot, the 128-pixel channel masks two): the
# smallest flow at the edge of k_net_lds's `split = np >= 2`
LOCAL = {'np2': _row((8, 16, 4), 3, *_RECT)}
GEN_ROWS = ROWS + list(LOCAL)
PATHS = ('default', 'streamed')
KNOB_CASES = [(n, o) for n in ('odd_d3', 'nk24', 'w12x20') for o in ('nogc', 'conv1')]
CASES = [(n, o) for n in GEN_ROWS for o in PATHS] + KNOB_CASES


def kw_of(name):
    """constructor arguments of cFlow / OracleCFlow / TorchCPUFlow: a preset, a sweep row or a local row"""
    if name in PRESETS:
        return PRESETS[name].kwargs()
    return dict(LOCAL[name], group_mode='reference') if name in LOCAL else _kw(name)


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    """test_shape_sweep._oracle (the sweep rows share its cache), the same for the local rows"""
    if name in SWEEP:
        return _oracle(name)
    kw = dict(kw_of(name), lambda_y=100.0)
    ora = OracleCFlow(**kw)
    P = ora.init_params(0)
    H, W, D = kw['io_shape']
    xy = np.random.default_rng(0).standard_normal((3, H, W, D)).astype(np.float32)
    zy_ref, ld_ref, abs_s = ora.forward(xy, P, abs_s=True)
    x_ref = ora.inverse(zy_ref, P)
    for a in (xy, zy_ref, ld_ref, abs_s, x_ref):
        a.setflags(write=False)
    return kw, ora, P, xy, zy_ref, ld_ref, abs_s, x_ref


def _randn(name, B, seed):
    H, W, D = kw_of(name)['io_shape']
    return np.random.default_rng(seed).standard_normal((B, H, W, D)).astype(np.float32)


# ---------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------

def _capi_kw(name):
    return {k: v for k, v in kw_of(name).items() if k != 'group_mode'}


def _couplings(lib, name):
    """(hc, wc) of every coupling layer of the row's plan"""
    rc, p, keep = _plan(lib, _capi_kw(name))
    assert rc == 0, lib.cnf_last_error()
    try:
        info = _lib.cnf_layer_info()
        out = []
        for li in range(lib.cnf_plan_num_layers(p)):
            assert lib.cnf_plan_layer_info(p, li, C.byref(info)) == 0
            if info.kind == 0:
                out.append((info.hc, info.wc))
        return out
    finally:
        lib.cnf_plan_destroy(p)


def _np_of(couplings):
    """the log-det slots per image and coupling (csrc/cnf_coupling.cpp ld_parts_for, maximum over the couplings)"""
    return max(max(1, min(16, (hc * wc + 63) // 64)) for hc, wc in couplings)


def test_coverage_claims(lib):
    """What the docstring says the rows reach, so that a planner or row change cannot silently empty it."""
    per_row = {n: _couplings(lib, n) for n in GEN_ROWS}
    nps = {n: _np_of(c) for n, c in per_row.items()}
    print('np per row:', nps)
    assert {1, 2, 3, 4, 16} <= set(nps.values())
    assert nps['np2'] == 2
    # spare k_coupling blocks / k_net_lds slots that have to be zeroed: a layer of at most 16 pixels in an np >= 3 flow
    assert any(nps[n] >= 3 and min(hc * wc for hc, wc in per_row[n]) <= 16 for n in GEN_ROWS)
    for n in ('min4x4', 'w12x20'):   # k_sample_fold's valid == false lanes
        H, W, _ = SWEEP[n]['io_shape']
        assert H * W * SWEEP[n]['x_d'] % 32 != 0, n
    H, W, D = SWEEP['min4x4']['io_shape']   # less than a wave per image in k_sample_logp / k_sample_ydev
    assert H * W * SWEEP['min4x4']['x_d'] < 64 and H * W * (D - SWEEP['min4x4']['x_d']) < 64
    assert min(SWEEP['r0']['ResNeXt_block_list']) == 0
    assert min(hc * wc for hc, wc in per_row['min4x4']) == 1


def _schedules(lib, name, path, B):
    rc, p, keep = _plan(lib, _capi_kw(name), options=_opt_str(_OPTS[path]))
    assert rc == 0, lib.cnf_last_error()
    try:
        inv = schedule_of_plan(lib, p, B, -1)
        ld = schedule_of_plan(lib, p, B, -2)
        assert schedule_of_plan(lib, p, B, -1) == inv   # (the -2 run left nothing behind)
        return inv, ld
    finally:
        lib.cnf_plan_destroy(p)


def test_schedule_with_logdet_is_the_inverse_plus_one_reduce(lib):
    """cnf_debug_schedule(-2) is the schedule of -1 followed by exactly one k_ld_reduce, on every case of the GPU
    part at B in (1, 3); across the rows the slot writers k_coupling, k_net_lds and k_map2 all occur."""
    seen = set()
    for name, path in CASES:
        for B in (1, 3):
            inv, ld = _schedules(lib, name, path, B)
            assert ld == inv + ['k_ld_reduce'], (name, path, B, inv, ld)
            seen.update(ld)
    for k in ('k_coupling', 'k_net_lds', 'k_map2'):
        assert k in seen, (k, sorted(seen))


# rows x regimes of the GPU part's "shapes x values"
VALUE_ROWS = ['w12x20', 'min4x4', 'odd_d3', 'odd_d5', 'nk24', 'nk48', 'rect32x48', 'np2', 'r0', 'r4', 'w2', 'wide']
VALUE_REGIMES = ['trained', 'negw', 'out30', 'lnoffset', 'lnconst1000']


class Ref:
    pass


@functools.lru_cache(maxsize=None)
def _ref64(name, regime):
    """float64 numpy oracle of a (row, regime) at B = 3, computed once and left unchanged: forward, the round
    trip of its own zy, and the inverse of zy cast to fp32 (the tensor the GPU and the fp32 graph get)."""
    r = Ref()
    r.kw = kw_of(name)
    r.ora = OracleCFlow(**r.kw)
    r.P = regime_params(r.ora, regime, seed=0)
    r.xy = _randn(name, 3, 0)
    with np.errstate(over='ignore'):
        r.zy, r.ld, r.abs_s = r.ora.forward(r.xy, r.P, abs_s=True)
        r.round_trip = _err(r.ora.inverse(r.zy, r.P), r.xy)
        r.z_in = r.zy.astype(np.float32)
        r.x = r.ora.inverse(r.z_in, r.P)
    for a in (r.xy, r.zy, r.ld, r.abs_s, r.z_in, r.x):
        a.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def _ref32(name, regime):
    """the fp32 torch-CPU graph on the identical inputs: (zy, per-image log-det, inverse of z_in)"""
    r = _ref64(name, regime)
    zy32, ld32, _, x32 = _torch_run(r.kw, r.P, r.xy, r.z_in, torch.float32)
    for a in (zy32, ld32, x32):
        a.setflags(write=False)
    return zy32, ld32, x32


@pytest.mark.parametrize('name', VALUE_ROWS)
def test_regime_is_finite_and_invertible_in_float64(name):
    """test_value_regimes' prerequisite on the rows: a regime the float64 flow cannot invert tests nothing."""
    for regime in VALUE_REGIMES:
        r = _ref64(name, regime)
        print(f'{name} {regime}: float64 round trip {r.round_trip:.2e}')
        assert np.isfinite(r.zy).all() and np.isfinite(r.ld).all() and np.isfinite(r.x).all(), regime
        assert r.round_trip <= 1e-9, (regime, r.round_trip)


# ---------------------------------------------------------------------------------------------
# GPU 1: inverse log-det against the oracle
# ---------------------------------------------------------------------------------------------

def _t(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize('name,path', CASES)
def test_inverse_logdet_matches_oracle(gpu, name, path):
    """x within 1e-5 of xy, -logdet within check_logdet's bound of the float64 forward log-det at xy, x the plain
    inverse's bit for bit, and the layer-by-layer walk: the same x, logdet as the forward's walk agrees
    (test_layerwise_equals_fused: rtol 1e-6, atol 1e-5). Worst err/tol: DESIGN.md (inverse log-det)."""
    kw, ora, P, xy, zy_ref, ld_ref, abs_s, x_ref = oracle_of(name)
    flow = _flow(kw, P, gpu, _OPTS[path])
    z = _t(zy_ref, gpu)
    x, ld = flow(z, -1, inverse_logdet=True)
    x0 = flow(z, -1)
    x2, ld2 = flow(z, -1, inverse_logdet=True, layerwise=True)
    torch.cuda.synchronize()
    assert ld.shape == (len(xy),) and ld.dtype == torch.float32
    assert torch.isfinite(x).all() and torch.isfinite(ld).all()
    e = _err(x.cpu().numpy(), xy)
    print(f'{name} {path}: inverse rel err {e:.3e} (err/tol {e / RTOL:.3f})')
    assert e < RTOL
    check_logdet(-ld.cpu().numpy().astype(np.float64), ld_ref, abs_s, f'{name} {path} inverse')
    assert same_bits(x, x0), 'x differs from the plain inverse'
    assert same_bits(x2, x0), 'the layerwise x differs'
    assert torch.allclose(ld, ld2, rtol=1e-6, atol=1e-5), (ld, ld2)


# ---------------------------------------------------------------------------------------------
# GPU 2: nothing but the image decides its log-det
# ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('path', PATHS)
@pytest.mark.parametrize('name', ['nk48', 'rect32x48', 'odd_d3', 'w12x20', 'np2', 'min4x4', 'r0'])
def test_logdet_depends_on_the_image_alone(gpu, name, path):
    """One batch of 7 against the same images in batches of 3 (the last one ragged): x and logdet bit-equal; the
    same after every workspace was filled with 0xFF bytes (every slot a NaN) and after a forward of another batch
    left its own sums in the slots."""
    kw, ora, P = oracle_of(name)[:3]
    flow = _flow(kw, P, gpu, _OPTS[path])
    z = flow(_t(_randn(name, 7, 5), gpu), 1)[0]
    x7, ld7 = flow(z, -1, inverse_logdet=True)
    torch.cuda.synchronize()
    assert torch.isfinite(x7).all() and torch.isfinite(ld7).all()
    other = _t(_randn(name, 7, 11), gpu)

    def check(what):
        for parts in ([(0, 7)], [(0, 3), (3, 6), (6, 7)]):
            for a, b in parts:
                x, ld = flow(z[a:b].contiguous(), -1, inverse_logdet=True)
                torch.cuda.synchronize()
                assert same_bits(x, x7[a:b]), f'{name} {path} {what} [{a}:{b}]: x differs'
                assert same_bits(ld, ld7[a:b]), f'{name} {path} {what} [{a}:{b}]: logdet differs ({ld} vs {ld7[a:b]})'

    check('as it is')
    for B in (7, 3, 1):
        flow._workspace(B).fill_(0xFF)
    check('NaN workspace')
    for B in (7, 3, 1):
        flow(other[:B].contiguous(), 1)
    check('after a forward')


# ---------------------------------------------------------------------------------------------
# GPU 3: the known-answer law grid in the inverse
# ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('variant', range(LAW_VARIANTS))
@pytest.mark.parametrize('name', ['tiny', 'small', 'np2', 'w12x20'])
def test_law_grid_in_the_inverse(gpu, name, variant):
    """test_value_regimes.law_params makes s = w tanh(bias) a known answer whatever the input: -logdet of the fused,
    the layer-by-layer and the streamed inverse against the oracle's log-det under LAW_LD sum|s|."""
    kw = kw_of(name)
    ora = OracleCFlow(**kw)
    P, _ = law_params(ora, variant)
    zy = _randn(name, 3, 100 + variant)
    _, ld_ref, abs_s = ora.forward(zy, P, abs_s=True)   # (s does not depend on the input)
    z = _t(zy, gpu)
    flow, streamed = _flow(kw, P, gpu), _flow(kw, P, gpu, {'NETLDS': 0})
    runs = {'fused': flow(z, -1, inverse_logdet=True), 'layerwise': flow(z, -1, inverse_logdet=True, layerwise=True),
            'streamed': streamed(z, -1, inverse_logdet=True)}
    torch.cuda.synchronize()
    worst = 0.0
    for what, (x, ld) in runs.items():
        assert torch.isfinite(x).all() and torch.isfinite(ld).all(), what
        e = np.abs(-ld.cpu().numpy().astype(np.float64) - ld_ref)
        worst = max(worst, float(np.max(e / np.maximum(LAW_LD * abs_s, 1e-300))))
        assert np.all(e <= LAW_LD * abs_s), (what, e, LAW_LD * abs_s)
    print(f'law grid {name} variant {variant}: inverse log-det worst err/bound {worst:.3f}')
    assert same_bits(runs['fused'][0], runs['layerwise'][0]) and same_bits(runs['fused'][0], runs['streamed'][0])


# ---------------------------------------------------------------------------------------------
# GPU 4: shapes x values
# ---------------------------------------------------------------------------------------------

# The per-image log-det bound 1e-5 max(|ref|, sum|s|) stays as it is except in these two regimes, where it takes
# the max(existing, K_FP32 e_32) form of zy and the inverse, because on the rows the fp32 torch-CPU graph alone
# misses or grazes the plain bound. Its own err/tol, worst row: lnoffset forward 0.83 (w2; 1.28 on another
# host), at the GPU's x 1.18 (w2), r4 0.98; lnconst1000 3.31 (nk24), odd_d5 2.31, np2 2.09. The GPU: lnoffset
# 0.42 forward / 0.43 inverse (it would pass the plain bound there), lnconst1000 2.69. lnconst1000 is
# test_value_regimes.LOGDET_FP32_FORM's case on the presets. In every other regime the fp32 graph and the GPU
# are at or below 0.01 of the bound.
LOGDET_FP32_FORM = ('lnoffset', 'lnconst1000')


def _ld_bound(regime, ld_ref, abs_s, e32):
    tol = ld_tol(ld_ref, abs_s)
    return np.maximum(tol, K_FP32 * e32) if regime in LOGDET_FP32_FORM else tol


def _check_fp32_form(what, label, got, got32, ref):
    """per image e_gpu <= max(RTOL, K_FP32 e_32), every figure printed first"""
    e_gpu, e_32 = _err_img(got, ref), _err_img(got32, ref)
    bound = np.maximum(RTOL, K_FP32 * e_32)
    above = e_gpu > RTOL
    ratio = float(np.max(e_gpu[above] / np.maximum(e_32[above], 1e-30))) if above.any() else 0.0
    print(f'{what} {label}: e_gpu {e_gpu.max():.3e} e_32 {e_32.max():.3e} worst e_gpu/bound '
          f'{np.max(e_gpu / bound):.3f} e_gpu/e_32 {np.max(e_gpu / np.maximum(e_32, 1e-30)):.2f} '
          f'(above {RTOL:g}: {ratio:.2f})')
    assert np.all(e_gpu <= bound), (what, label, e_gpu, bound)


VALUE_CASES = [(n, r, p) for n in VALUE_ROWS for r in VALUE_REGIMES for p in PATHS]


@pytest.mark.gpu
@pytest.mark.parametrize('name,regime,path', VALUE_CASES)
def test_values_off_initialisation_on_the_rows(gpu, name, regime, path):
    """test_value_regimes.test_forward_logdet_inverse_match_oracle on the sweep's rows, with the inverse's log-det:
    zy per image within max(RTOL, K_FP32 e_32) of float64 (e_32: the fp32 torch-CPU graph on the identical inputs);
    the forward log-det under _ld_bound; the inverse's log-det against the float64 forward at the GPU's own x (so
    the inverse's ill-conditioning does not enter), the fp32 yardstick at that same x. (x itself: the next test.)"""
    r = _ref64(name, regime)
    zy32, ld32, x32 = _ref32(name, regime)
    flow = _flow(r.kw, r.P, gpu, _OPTS[path])
    zy, ld = flow(_t(r.xy, gpu), 1, per_image_logdet=True)
    x, ldi = flow(_t(r.z_in, gpu), -1, inverse_logdet=True)
    torch.cuda.synchronize()
    for t in (zy, ld, x, ldi):
        assert torch.isfinite(t).all()
    what = f'{name} {regime} {path}'
    _check_fp32_form(what, 'zy', zy.cpu().numpy(), zy32, r.zy)
    e, e32 = np.abs(ld.cpu().numpy().astype(np.float64) - r.ld), np.abs(ld32 - r.ld)
    tol = ld_tol(r.ld, r.abs_s)
    print(f'{what} logdet: worst err/tol {np.max(e / tol):.3f} (fp32 reference {np.max(e32 / tol):.3f})')
    assert np.all(e <= _ld_bound(regime, r.ld, r.abs_s, e32)), (what, e, tol)
    # inverse log-det: float64 and fp32 forward at the GPU's own x
    x_gpu = x.cpu().numpy()
    with np.errstate(over='ignore'):
        _, ld_at_x, abs_s_at_x = r.ora.forward(x_gpu.astype(np.float64), r.P, abs_s=True)
    ld32_at_x = _torch_run(r.kw, r.P, x_gpu, r.z_in[:1], torch.float32)[1]
    e, e32 = np.abs(-ldi.cpu().numpy().astype(np.float64) - ld_at_x), np.abs(ld32_at_x - ld_at_x)
    tol = ld_tol(ld_at_x, abs_s_at_x)
    print(f'{what} inverse logdet: worst err/tol {np.max(e / tol):.3f} (fp32 reference {np.max(e32 / tol):.3f})')
    assert np.all(e <= _ld_bound(regime, ld_at_x, abs_s_at_x, e32)), (what, e, tol)


# The one case of the 120 whose inverse misses max(RTOL, K_FP32 e_32): image 0, e_gpu 4.79e-4 = 11.45 e_32 (NETLDS=0
# 1.49e-4, fp32 numpy 2.4e-5). test_inverse_error_by_layer below splits that error exactly into the layers' local
# errors carried through the float64 flow; figures and reading in DESIGN.md section 3 ("The regimes on the rows").
ILL_CONDITIONED = {('nk24', 'negw', 'default'): 'image 0: the first two layers of the inverse carry a local error of '
                   '2e-9 / 9e-8 (no larger than fp32 numpy\'s or NETLDS=0\'s there) to 1.8e-4 / 6.4e-4 of x; the fp32 '
                   'graphs\' two contributions, as large, cancel to 2.4e-5 .. 4.2e-5'}


@pytest.mark.gpu
@pytest.mark.parametrize('name,regime,path', [
    pytest.param(*c, marks=[pytest.mark.xfail(strict=True, reason=ILL_CONDITIONED[c])] if c in ILL_CONDITIONED else [])
    for c in VALUE_CASES])
def test_inverse_off_initialisation_on_the_rows(gpu, name, regime, path):
    """The inverse of the float64 zy cast to fp32, per image within max(RTOL, K_FP32 e_32) of the float64 inverse."""
    r = _ref64(name, regime)
    x = _flow(r.kw, r.P, gpu, _OPTS[path])(_t(r.z_in, gpu), -1)
    assert torch.isfinite(x).all()
    _check_fp32_form(f'{name} {regime} {path}', 'inverse', x.cpu().numpy(), _ref32(name, regime)[2], r.x)


def _inverse_from(ora, P, z_in, replace=None, stop_at=None):
    """OracleCFlow.inverse in float64 with the output of coupling replace[0] replaced by replace[1]; with stop_at,
    the input of coupling stop_at instead of x"""
    vu, zy = np.asarray(z_in, np.float64), None
    for e in ora.sf_layers:
        vu, zy = (O.squeeze_forward if e.kind == 'squeeze' else O.factor_forward)(vu, zy)
    for e in reversed(ora.layers):
        if e.kind == 'coupling':
            if e.coupling.index == stop_at:
                return vu
            vu = O.coupling_backward(vu, e.coupling, P, ora.ksize, ora.ln)
            if replace is not None and e.coupling.index == replace[0]:
                vu = np.asarray(replace[1], np.float64)
        elif e.kind == 'squeeze':
            vu, zy = O.squeeze_backward(vu, zy)
        else:
            vu, zy = O.factor_backward(vu, zy, e.num_prev_factors)
    return vu


def _img_max(a):
    return np.max(np.abs(a).reshape(len(a), -1), axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize('path', PATHS)
@pytest.mark.parametrize('name,regime', [('nk24', 'negw'), ('wide', 'negw')])
def test_inverse_error_by_layer(gpu, name, regime, path):
    """Where the end-to-end inverse exceeds 1e-5, what each layer adds. With a_k the GPU's output of coupling k in
    the layer-by-layer walk (its x is the fused call's, bit for bit), L_k the float64 layer and R_k the float64
    flow after it, x_gpu - x_64 = sum_k [R_k(a_k) - R_k(L_k(a_{k-1}))] exactly: each term is layer k's local error
    on the input it really got, carried to x by the rest of the flow. Asserted: the identity (to 1e-9 of |x|),
    so the attribution printed is the whole error; and per layer and image the local error within
    max(RTOL, K_FP32 e_32), e_32 the fp32 numpy layer on the identical input -- the bound of the end-to-end
    check where one layer's conditioning (at most e^3) is all that enters. A layer that errs shows here whatever
    the image's conditioning; the amplification R_k applies is printed, not asserted."""
    r = _ref64(name, regime)
    P64, P32 = r.ora._cast(r.P, np.float64), r.ora._cast(r.P, np.float32)
    flow = _flow(r.kw, r.P, gpu, _OPTS[path])
    z = _t(r.z_in, gpu)
    x = flow(z, -1)
    # cFlow._call_layerwise_inverse, recording every coupling's output
    uv, zy = z, None
    for layer in flow.squeeze_factor_layers_list:
        uv, _, zy = layer.forward_and_Jacobian(uv, None, zy)
    acts = {}
    for layer in reversed(flow.layers_list):
        uv, zy = layer.backward(uv, zy)
        if hasattr(layer, 'coupling_index'):
            acts[layer.coupling_index] = uv.cpu().numpy()
    assert same_bits(uv, x), 'the layer-by-layer x differs from the fused one'
    x = x.cpu().numpy().astype(np.float64)
    scale = _img_max(r.x)
    total, acc, prev = x - r.x, np.zeros_like(r.x), None
    for c in [e.coupling for e in reversed(r.ora.layers) if e.kind == 'coupling']:
        v_in = _inverse_from(r.ora, P64, r.z_in, replace=prev, stop_at=c.index)   # (a_{k-1} through the layout layers)
        exact = O.coupling_backward(v_in, c, P64, r.ora.ksize, r.ora.ln)
        u32 = O.coupling_backward(v_in.astype(np.float32), c, P32, r.ora.ksize, r.ora.ln)
        a_k = acts[c.index].astype(np.float64)
        contrib = _inverse_from(r.ora, P64, r.z_in, replace=(c.index, a_k)) - \
            _inverse_from(r.ora, P64, r.z_in, replace=(c.index, exact))
        acc += contrib
        e_gpu, e_32 = _err_img(a_k, exact), _err_img(u32, exact)
        carried = _img_max(contrib) / scale
        print(f'{name} {regime} {path} c{c.index:02d}: local e_gpu {np.array2string(e_gpu, precision=2)} e_32 '
              f'{np.array2string(e_32, precision=2)} carried to x {np.array2string(carried, precision=2)} '
              f'(x {np.array2string(carried / np.maximum(e_gpu, 1e-30), precision=0)})')
        assert np.all(e_gpu <= np.maximum(RTOL, K_FP32 * e_32)), (c.index, e_gpu, e_32)
        prev = (c.index, a_k)
    print(f'{name} {regime} {path}: end to end {np.array2string(_img_max(total) / scale, precision=3)}')
    assert np.all(_img_max(acc - total) <= 1e-9 * scale), _img_max(acc - total) / scale


# ---------------------------------------------------------------------------------------------
# GPU 5: sampling on the rows
# ---------------------------------------------------------------------------------------------

SAMPLE_CASES = [(n, {}) for n in ('min4x4', 'w12x20', 'odd_d3', 'r4', 'np2', 'rect32x48')] + \
               [('r4', dict(residual=True)), ('r4', dict(logit_a=0.01)), ('r4', dict(logit_a=0.01, residual=True))]
OUTPUTS = ('samples', 'mean', 'std', 'y_dev')


@pytest.mark.gpu
@pytest.mark.parametrize('name,post', SAMPLE_CASES, ids=['-'.join([n] + list(p)) for n, p in SAMPLE_CASES])
def test_sampling_on_the_rows(gpu, name, post):
    """B = 3 conditions, S = 5 draws: the samples are the inverse of the documented latent bit for bit (through
    the post-transforms: 1e-5 of the float64 oracle's); no output depends on chunk or on whether log_prob is
    asked for; log_prob composes from zy and the inverse's log-det within one fp32 ulp and agrees with float64;
    y_dev and mean / std under the bounds of tests/test_sampling.py."""
    kw, ora, P = oracle_of(name)[:3]
    flow = _flow(kw, P, gpu)
    B, S, x_d = 3, 5, kw['x_d']
    H, W, D = kw['io_shape']
    y_np = np.ascontiguousarray(_randn(name, B, 21)[..., x_d:])
    y = _t(y_np, gpu)
    args = dict(temperature=0.9, seed=7, offset=2, return_y_dev=True, **post)
    what = f'{name} {post or ""}'
    zy = _zy_kw(kw, y, S, 0.9, seed=7, offset=2)
    xy_hat = flow(zy, -1)
    ref = None
    for chunk in (1, 4, 7, B * S, 64):
        got = flow.sample(y, S, chunk=chunk, return_log_prob=True, **args)
        plain = flow.sample(y, S, chunk=chunk, **args)
        assert sorted(got) == ['log_prob', 'mean', 'samples', 'std', 'y_dev'] and sorted(plain) == sorted(OUTPUTS)
        for t in got.values():
            assert torch.isfinite(t).all()
        ref = got if ref is None else ref
        for n in OUTPUTS + ('log_prob',):
            assert same_bits(got[n], ref[n]), f'{what} chunk={chunk}: {n} differs from chunk=1'
        for n in OUTPUTS:
            assert same_bits(plain[n], ref[n]), f'{what} chunk={chunk}: {n} differs in the call without log_prob'
    # the draws: the inverse of the documented latent
    draws = xy_hat[..., :x_d].reshape(B, S, H, W, x_d)
    x64 = ora.inverse(zy.cpu().numpy(), P)
    want = x64[..., :x_d].reshape(B, S, H, W, x_d)
    if 'logit_a' in post:
        want = transforms_np.de_logitify(want, post['logit_a'])
    if post.get('residual'):
        want = want + y_np.astype(np.float64)[:, None]
    if not post:
        assert same_bits(ref['samples'], draws), f'{what}: samples are not the inverse of the documented latent'
    e = _err(ref['samples'].cpu().numpy(), want)
    print(f'{what}: samples rel err {e:.3e}')
    assert e < RTOL
    # log_prob: the flow's input space, so the post-transforms do not enter
    expected, bound = _composed_kw(kw, flow, zy, B, S)
    lp = ref['log_prob'].cpu().numpy().astype(np.float64)
    d = np.abs(lp - expected.astype(np.float64))
    print(f'{what}: worst |log_prob - composed| / ulp bound {np.max(d / bound):.3f}')
    assert np.all(d <= bound), (d, bound)
    lp_ref, tol = log_prob_oracle(ora, P, zy.cpu().numpy(), x_d)
    e = np.abs(lp.reshape(-1) - lp_ref)
    print(f'{what}: log_prob max abs err {e.max():.3e}, worst err/tol {np.max(e / tol):.3f}')
    assert np.all(e <= tol), (e, tol)
    # y_dev: float64 sum |y_hat - y| of the GPU's own inverse output, 1e-5 of the sum (test_sampling.test_y_dev)
    y64 = np.repeat(y_np.astype(np.float64), S, axis=0)
    dev = np.abs(xy_hat.cpu().numpy().astype(np.float64)[..., x_d:] - y64).reshape(B * S, -1).sum(1).reshape(B, S)
    e = np.abs(ref['y_dev'].cpu().numpy().astype(np.float64) - dev)
    print(f'{what}: y_dev worst err/bound {np.max(e / (RTOL * dev)):.3e}')
    assert dev.min() > 0 and np.all(e <= RTOL * dev)
    std = _check_stats(ref, what)
    assert std.max() > 1e-3


# ---------------------------------------------------------------------------------------------
# GPU 6: more than FOLD_BATCH = 64 draws of a condition in one chunk
# ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('name', ['tiny', 'min4x4'])
def test_more_than_64_draws_per_chunk(gpu, name):
    """k_sample_fold's loop over batches of 64 draws. S = 70 in one chunk of 140: two batches, the second short
    (6 draws), the first-draw flag in the first only. S = 130, chunk = 100: a chunk holding 100 draws of one
    condition, then 30 carried ones and 70 of the next. S = 170, chunk = 100: a carried state (s0 = 100) followed
    by 70 draws, two batches. Each against chunk = 5, where no batch exceeds 5 draws: samples, mean, std bit-equal,
    and mean / std within stats_bounds of the float64 statistics of the returned samples."""
    kw = kw_of(name)
    ora = OracleCFlow(**kw)
    flow = _flow(kw, ora.init_params(0), gpu)
    x_d = kw['x_d']
    y = _t(_randn(name, 2, 22)[..., x_d:], gpu)
    for S, chunk in ((70, 140), (130, 100), (170, 100)):
        got = flow.sample(y, S, seed=3, chunk=chunk)
        ref = flow.sample(y, S, seed=3, chunk=5)
        for n in ('samples', 'mean', 'std'):
            assert torch.isfinite(got[n]).all(), (S, chunk, n)
            assert same_bits(got[n], ref[n]), f'{name} S={S}: {n} differs between chunk={chunk} and chunk=5'
        std = _check_stats(got, f'{name} S={S} chunk={chunk}')
        assert std.max() > 1e-3
