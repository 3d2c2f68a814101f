"""Conditional sampling: cnf_flow_sample / cFlow.sample (include/cnf.h), the recipe of TOYcINN.py:807-817
(z from the prior, concat the condition y, the model in the generative direction) with the post-transforms
and the per-pixel mean / std over the draws.

CPU part (host only, against the cross-compiled library): every argument error is CNF_E_INVALID with a
message before any HIP call, and the sample workspace has the documented size.

GPU part: the latent is the documented Philox stream (bit for bit against renew_noise + cat + the inverse);
no result depends on the chunking, bit for bit; the draws agree with the float64 oracle's inverse under the
project's 1e-5 bound; mean / std agree with the float64 statistics of the returned samples within a bound
derived from the fold's own operations (stats_bounds below, written before the first GPU run); y_dev; the
workspace contract of tests/test_state_independence.py on the new entry point; the moments of the draws.

Flows: the presets 'tiny' (8x8x2, x_d 1: y has x's depth, so the residual applies) and 'small' (16x16x4,
x_d 3), and the shape-sweep rows 'xd1of4' (x_d 1 of 4: three y channels) and 'odd_d5' (8x8x5: no 16-byte
alignment of a pixel, the element-wise k_latent). Weights OracleCFlow.init_params(0), y the y channels of
synthetic_class_batch."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from arl_conditional_normalizing_flows_amd import _lib
from arl_conditional_normalizing_flows_amd.config import PRESETS
from oracle import transforms_np
from oracle.cflow_np import OracleCFlow, synthetic_class_batch

from test_capi import _plan
from test_gpu_parity import RTOL, _err
from test_shape_sweep import SWEEP
from test_state_independence import PATTERNS, Buffers, assert_patterns_agree, max_diff, same_bits

FLOWS = {
    'tiny': PRESETS['tiny'].kwargs(),
    'small': PRESETS['small'].kwargs(),
    'xd1of4': dict(SWEEP['xd1of4'], group_mode='reference'),
    'odd_d5': dict(SWEEP['odd_d5'], group_mode='reference'),
}


def _capi_kw(name):
    return {k: v for k, v in FLOWS[name].items() if k != 'group_mode'}


def _desc(S=4, chunk=3, T=1.0, seed=0, offset=0, logit_a=0.0, residual=0):
    return _lib.cnf_sample_desc(S, chunk, T, seed, offset, logit_a, residual)


# ---------------------------------------------------------------------------------------------
# CPU: the C ABI's host side
# ---------------------------------------------------------------------------------------------

A, Y, WS, OUT = 1 << 40, 2 << 40, 3 << 40, 4 << 40   # placeholder device addresses, never dereferenced

ARG_ERRORS = [
    ('null_y', 'tiny', dict(y=None), {}, 'y'),
    ('S0', 'tiny', {}, dict(S=0), 'num_samples'),
    ('chunk0', 'tiny', {}, dict(chunk=0), 'chunk'),
    ('T_negative', 'tiny', {}, dict(T=-0.5), 'temperature'),
    ('T_inf', 'tiny', {}, dict(T=float('inf')), 'temperature'),
    ('T_nan', 'tiny', {}, dict(T=float('nan')), 'temperature'),
    ('logit_half', 'tiny', {}, dict(logit_a=0.5), 'logit_a'),
    ('logit_negative', 'tiny', {}, dict(logit_a=-0.01), 'logit_a'),
    ('residual_depth', 'small', {}, dict(residual=1), 'residual'),    # D - x_d = 1 != x_d = 3
    ('residual_depth3', 'xd1of4', {}, dict(residual=1), 'residual'),  # D - x_d = 3 != x_d = 1
    ('no_output', 'tiny', dict(samples=None, mean=None, std=None, y_dev=None), {}, 'output'),
    ('B0', 'tiny', dict(B=0), {}, 'B'),
]


@pytest.mark.parametrize('case,name,args,desc,word', ARG_ERRORS, ids=[c[0] for c in ARG_ERRORS])
def test_argument_errors(lib, case, name, args, desc, word):
    """CNF_E_INVALID and a message naming the argument, with nothing launched (no GPU here)."""
    rc, p, keep = _plan(lib, _capi_kw(name))
    assert rc == 0, lib.cnf_last_error()
    try:
        a = dict(y=Y, samples=OUT, mean=OUT + (1 << 30), std=OUT + (2 << 30), y_dev=OUT + (3 << 30), B=2)
        a.update(args)
        d = _desc(**desc)
        rc = lib.cnf_flow_sample(p, A, A, a['y'], C.byref(d), a['samples'], a['mean'], a['std'], a['y_dev'], WS,
                                 a['B'], None)
        msg = lib.cnf_last_error().decode()
        assert rc == -1 and msg, (case, rc, msg)
        assert word in msg, (case, msg)
        if not args:   # a descriptor error: no workspace size either
            assert lib.cnf_plan_sample_workspace_bytes(p, 2, C.byref(d)) == 0
    finally:
        lib.cnf_plan_destroy(p)


@pytest.mark.parametrize('name', list(FLOWS))
def test_sample_workspace_bytes(lib, name):
    """At least the inverse workspace of `chunk` images + the zy and xy_hat chunk buffers + the (K, S1, S2)
    state; non-decreasing in B and chunk; independent of S."""
    kw = _capi_kw(name)
    H, W, D = kw['io_shape']
    x_d = kw['x_d']
    rc, p, keep = _plan(lib, kw)
    assert rc == 0, lib.cnf_last_error()
    try:
        def size(B, S, chunk):
            d = _desc(S=S, chunk=chunk)
            return int(lib.cnf_plan_sample_workspace_bytes(p, B, C.byref(d)))
        for B, chunk in [(1, 1), (2, 3), (2, 64), (8, 64), (5, 7)]:
            need = int(lib.cnf_plan_workspace_bytes(p, chunk)) + 2 * chunk * H * W * D * 4 + 3 * B * H * W * x_d * 4
            got = size(B, 7, chunk)
            assert got >= need, (B, chunk, got, need)
            assert got <= need + 4 * 256, (B, chunk, got, need)   # (exactly that, up to the regions' 256-byte alignment)
            assert len({size(B, S, chunk) for S in (1, 2, 7, 64, 1000)}) == 1
        for chunk in (1, 3, 64):
            s = [size(B, 5, chunk) for B in range(1, 12)]
            assert s == sorted(s) and s[-1] > s[0]
        for B in (1, 4):
            s = [size(B, 5, chunk) for chunk in range(1, 70)]
            assert s == sorted(s) and s[-1] > s[0]
    finally:
        lib.cnf_plan_destroy(p)


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _flow(name, netlds=1, zero_last_conv=False):
    from arl_conditional_normalizing_flows_amd.make_model import cFlow
    kw = FLOWS[name]
    flow = cFlow(**kw, debug_options={'NETLDS': netlds})
    ora = OracleCFlow(**kw)
    P = ora.init_params(0, zero_last_conv=True) if zero_last_conv else ora.init_params(0)
    flow.set_weights(P)
    return flow, ora, P


@functools.lru_cache(maxsize=None)
def _y_np(name, B, seed=1):
    """the y channels of a synthetic_class_batch of the flow's shape (D - 1 uniform channels + the class plane)"""
    H, W, D = FLOWS[name]['io_shape']
    xy = synthetic_class_batch(B, H, W, D - 1, seed=seed)
    return np.ascontiguousarray(xy[..., FLOWS[name]['x_d']:])


def _y(name, B, seed=1):
    return torch.from_numpy(_y_np(name, B, seed).copy()).cuda()


def _zy(name, y, S, T, seed, offset):
    """the documented latent by the parent commit's means: renew_noise of [B,S,H,W,x_d], times T, cat y"""
    from arl_conditional_normalizing_flows_amd.base_functions import renew_noise
    H, W, D = FLOWS[name]['io_shape']
    B, x_d = y.shape[0], FLOWS[name]['x_d']
    z = renew_noise(torch.empty((B, S, H, W, x_d), device=y.device), seed=seed, offset=offset)
    yb = y[:, None].expand(B, S, H, W, D - x_d)
    return torch.cat([T * z, yb], dim=-1).reshape(B * S, H, W, D).contiguous()


LATENT_CASES = [('tiny', 1), ('small', 1), ('xd1of4', 1), ('odd_d5', 1), ('small', 0)]


@pytest.mark.gpu
@pytest.mark.parametrize('name,netlds', LATENT_CASES, ids=[f'{n}{"" if l else "-streamed"}' for n, l in LATENT_CASES])
def test_latent_is_the_documented_stream(gpu, name, netlds):
    """samples == flow(cat(T * renew_noise, y), -1)[..., :x_d] bit for bit, at T in {1, 0.7, 0} and chunks
    {1, 3, 14, 64} of the 14 images of B = 2, S = 7 (3: chunks 3, 3, 3, 3, 2, straddling the two conditions)."""
    flow, ora, P = _flow(name, netlds)
    B, S, x_d = 2, 7, FLOWS[name]['x_d']
    y = _y(name, B)
    for T in (1.0, 0.7, 0.0):
        zy = _zy(name, y, S, T, seed=5, offset=3)
        ref = flow(zy, -1)[..., :x_d].reshape(B, S, *zy.shape[1:3], x_d)
        assert torch.isfinite(ref).all()
        for chunk in (1, 3, 14, 64):
            got = flow.sample(y, S, temperature=T, seed=5, offset=3, chunk=chunk, return_stats=False)['samples']
            assert got.shape == ref.shape
            assert torch.equal(got, ref), f'{name} T={T} chunk={chunk}: max abs diff {max_diff(got, ref):.3e}'
    # the default chunk, and one condition given as [H, W, D - x_d]
    zy = _zy(name, y[:1], S, 1.0, seed=5, offset=0)
    got = flow.sample(y[0], S, seed=5)['samples']
    assert torch.equal(got, flow(zy, -1)[..., :x_d].reshape(got.shape))


CHUNK_CASES = [('tiny', dict(logit_a=0.01, residual=True)), ('small', {}), ('xd1of4', dict(logit_a=0.01)), ('odd_d5', {})]


@pytest.mark.gpu
@pytest.mark.parametrize('name,kw', CHUNK_CASES, ids=[c[0] for c in CHUNK_CASES])
def test_results_do_not_depend_on_chunk(gpu, name, kw):
    """samples, mean, std, y_dev bit-equal across chunk in {1, 3, 5, 14}, with and without the samples output,
    and from one call to the next; seed and offset select the draws; the stream is one stream."""
    flow, ora, P = _flow(name)
    B, S = 2, 7
    H, W, D = FLOWS[name]['io_shape']
    x_d = FLOWS[name]['x_d']
    y = _y(name, B)
    names = ('samples', 'mean', 'std', 'y_dev')

    def run(**over):
        a = dict(seed=9, offset=11, chunk=14, return_y_dev=True, **kw)
        a.update(over)
        return flow.sample(y, S, **a)
    ref = run()
    assert sorted(ref) == sorted(names)
    for n in names:
        assert torch.isfinite(ref[n]).all(), n
    for chunk in (1, 3, 5, 14):
        for rs in (True, False):
            got = run(chunk=chunk, return_samples=rs)
            assert sorted(got) == sorted(n for n in names if rs or n != 'samples')
            for n, t in got.items():
                assert same_bits(t, ref[n]), f'{name} chunk={chunk} return_samples={rs}: {n} differs, ' \
                                             f'max abs diff {max_diff(t, ref[n]):.3e}'
    again = run()
    for n in names:
        assert same_bits(again[n], ref[n]), n
    assert not torch.equal(run(seed=10)['samples'], ref['samples'])
    assert not torch.equal(run(offset=12)['samples'], ref['samples'])
    # offset + H W x_d: draw s + 1 of b becomes draw s
    shifted = run(offset=11 + H * W * x_d)['samples']
    assert torch.equal(shifted[:, :-1], ref['samples'][:, 1:])
    # the outputs asked for, and only those
    assert sorted(flow.sample(y, S, return_samples=False, return_stats=False, return_y_dev=True)) == ['y_dev']
    with pytest.raises(AssertionError):
        flow.sample(y, S, return_samples=False, return_stats=False)
    with pytest.raises(AssertionError):
        flow.sample(y, 0)


@functools.lru_cache(maxsize=None)
def _oracle_draws(name, B, S, T, seed, offset):
    """float64 inverse of the documented zy (the latent read back from the GPU's renew_noise): [B,S,H,W,D]"""
    flow, ora, P = _flow(name)
    zy = _zy(name, _y(name, B), S, T, seed, offset).cpu().numpy()
    xy = ora.inverse(zy, P)
    return xy.reshape(B, S, *xy.shape[1:])


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['tiny', 'small'])
@pytest.mark.parametrize('T', [1.0, 0.7])
def test_draws_match_oracle(gpu, name, T):
    """OracleCFlow.inverse (float64) of the same zy against the samples: 1e-5 relative (test_gpu_parity._err);
    numpy fp32 against float64 on these inputs is at 2.6e-7 .. 3.2e-7. The same with logit_a = 0.01 through
    oracle/transforms_np.de_logitify of the oracle's draws, and with the residual on the D = 2 x_d flow."""
    flow, ora, P = _flow(name)
    B, S, x_d = 2, 3, FLOWS[name]['x_d']
    y = _y(name, B)
    ref = _oracle_draws(name, B, S, T, 4, 0)[..., :x_d]
    cases = [('plain', {}, ref), ('logit', dict(logit_a=0.01), transforms_np.de_logitify(ref, 0.01))]
    if name == 'tiny':
        y64 = _y_np(name, B).astype(np.float64)[:, None]
        cases.append(('residual', dict(residual=True), ref + y64))
        cases.append(('logit+residual', dict(logit_a=0.01, residual=True), transforms_np.de_logitify(ref, 0.01) + y64))
    for what, kw, r in cases:
        got = flow.sample(y, S, temperature=T, seed=4, return_stats=False, **kw)['samples'].cpu().numpy()
        e = _err(got, r)
        print(f'{name} T={T} {what}: rel err {e:.3e}')
        assert e < RTOL, (what, e)


U = 2.0 ** -24   # unit roundoff of fp32


def _gamma(k):
    return k * U / (1.0 - k * U)


def stats_bounds(samples):
    """Bounds on |mean_gpu - mean| and |std_gpu - std| against the exact statistics of the fp32 samples
    [B,S,...], from the operations of sample_fold / sample_finish (csrc/cnf_device.h) on the S draws v_0 ..
    v_{S-1} of one element, u = 2^-24, gamma_k = k u / (1 - k u), m = S - 1:

      K  = v_0                                  exact
      d_i = fl(v_i - K)                         = (v_i - K)(1 + delta), |delta| <= u
      S1 = fl-sum of d_1 .. d_m in order        |S1 - T1| <= gamma_m A1 =: E1     (m - 1 additions after the
                                                first, which adds to 0 exactly, + the rounding of each d_i)
           with T1 = sum (v_i - K), A1 = sum |v_i - K|
      S2 = fma(d_i, d_i, S2) in order           |S2 - A2| <= gamma_{m+2} A2 =: E2 (one rounding per fma, and
           with A2 = sum (v_i - K)^2            d_i^2 carries (1 + delta)^2)
      mean = fl(K + fl(S1 / S))                 division and sqrt are taken as faithful (1 ulp: relative 2u),
                                                so the bound does not rest on the compiler's division flag
           e_div  = E1 / S + 2u (|T1| + E1) / S
           e_mean = e_div + u (|mean| + e_div)
      q  = fl(fl(S1 S1) / S)                    Eq = (2 |T1| E1 + E1^2) / S + gamma_3 (|T1| + E1)^2 / S
      r  = fl(S2 - q)                           Er = (E2 + Eq)(1 + u) + u V,  V = A2 - T1^2 / S = S var
      w  = max(0, fl(r / S))                    Ew = Er / S + 2u (var + Er / S)   (the clamp moves w towards var >= 0)
      std = fl(sqrt(w))                         |sqrt(w) - sqrt(var)| <= min(Ew / std, sqrt(Ew)) =: a
           e_std = a + 2u (std + a)

    Everything is relative to |v - K|, the spread around the first draw, never to |v| (only the final
    addition K + S1/S rounds at the size of the mean): a fold around 0 instead of K has e_std of order
    u mean^2 / std. T1, A1, A2 are evaluated in float64 (their own rounding, 1e-16 relative, is 8 orders
    below u). Returns (mean, std, e_mean, e_std), float64 arrays over the elements."""
    v = np.asarray(samples, np.float64)
    S = v.shape[1]
    m = S - 1
    dk = v - v[:, :1]
    T1, A1, A2 = dk.sum(1), np.abs(dk).sum(1), (dk * dk).sum(1)
    mean, std = v.mean(1), v.std(1)
    var = std * std
    E1 = _gamma(m) * A1
    E2 = _gamma(m + 2) * A2
    e_div = E1 / S + 2 * U * (np.abs(T1) + E1) / S
    e_mean = e_div + U * (np.abs(mean) + e_div)
    Eq = (2 * np.abs(T1) * E1 + E1 * E1) / S + _gamma(3) * (np.abs(T1) + E1) ** 2 / S
    Er = (E2 + Eq) * (1 + U) + U * np.maximum(A2 - T1 * T1 / S, 0.0)
    Ew = Er / S + 2 * U * (var + Er / S)
    with np.errstate(divide='ignore', invalid='ignore'):
        a = np.minimum(np.where(std > 0, Ew / std, np.inf), np.sqrt(Ew))
    e_std = a + 2 * U * (std + a)
    return mean, std, e_mean, e_std


def _check_stats(out, what):
    mean, std, e_mean, e_std = stats_bounds(out['samples'].cpu().numpy())
    dm = np.abs(out['mean'].cpu().numpy().astype(np.float64) - mean)
    ds = np.abs(out['std'].cpu().numpy().astype(np.float64) - std)
    # error over bound, 0 / 0 (an exact result with a zero bound) counted as 0
    rm = np.max(np.where(dm > 0, dm / np.where(e_mean > 0, e_mean, 1e-300), 0.0))
    rs = np.max(np.where(ds > 0, ds / np.where(e_std > 0, e_std, 1e-300), 0.0))
    print(f'{what}: mean worst err/bound {rm:.3f} (max err {dm.max():.3e}), std worst err/bound {rs:.3f} '
          f'(max err {ds.max():.3e}, std <= {std.max():.3e})')
    assert np.all(dm <= e_mean), (what, rm)
    assert np.all(ds <= e_std), (what, rs)
    return std


STATS_CASES = [('tiny', 2, 7, 1.0, {}), ('tiny', 1, 64, 1.0, {}), ('small', 2, 7, 0.7, dict(logit_a=0.01)),
               ('odd_d5', 2, 33, 1.0, {}), ('xd1of4', 3, 2, 1.0, {}), ('tiny', 2, 7, 1.0, dict(residual=True))]


@pytest.mark.gpu
@pytest.mark.parametrize('name,B,S,T,kw', STATS_CASES,
                         ids=['-'.join([n, f'B{B}', f'S{S}'] + list(kw)) for n, B, S, T, kw in STATS_CASES])
def test_mean_and_std_of_the_draws(gpu, name, B, S, T, kw):
    """mean / std against the float64 np.mean / np.std(ddof=0) of the returned fp32 samples (the kernel's own
    input, so the tested quantity is the reduction), within stats_bounds; a chunk that cuts the draws."""
    flow, ora, P = _flow(name)
    out = flow.sample(_y(name, B), S, temperature=T, seed=2, chunk=5, **kw)
    std = _check_stats(out, f'{name} B={B} S={S} T={T} {kw}')
    assert std.max() > 1e-3   # the draws do differ


@pytest.mark.gpu
def test_stats_edge_cases_are_exact(gpu):
    flow, ora, P = _flow('small')
    y = _y('small', 2)
    out = flow.sample(y, 1, seed=3)                          # S = 1
    assert torch.equal(out['std'], torch.zeros_like(out['std']))
    assert same_bits(out['mean'], out['samples'][:, 0])
    out = flow.sample(y, 5, temperature=0.0, seed=3, chunk=3)   # T = 0: every draw is the mode's image
    for s in range(1, 5):
        assert same_bits(out['samples'][:, s], out['samples'][:, 0])
    assert torch.equal(out['std'], torch.zeros_like(out['std']))
    assert same_bits(out['mean'], out['samples'][:, 0])


@pytest.mark.gpu
def test_std_survives_a_large_offset(gpu):
    """residual=True with y + 1000: the draws sit at 1000 with a spread of order 1, and std stays within the same
    derived bound of the float64 value (of order 1e-6 here; sums around 0 instead of around the first draw
    err by u mean^2 / std, of order 1e-2)."""
    flow, ora, P = _flow('tiny')
    y = _y('tiny', 2) + 1000.0
    out = flow.sample(y, 7, seed=2, chunk=5, residual=True)
    assert torch.isfinite(out['samples']).all() and float(out['samples'].min()) > 900.0
    std = _check_stats(out, 'tiny residual y+1000')
    assert std.max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(FLOWS))
def test_y_dev(gpu, name):
    """y_dev[b, s] against the float64 sum |xy_hat[..., x_d:] - y| of the GPU's own inverse output: 1e-5 of the
    sum (the NLL terms' bar)."""
    flow, ora, P = _flow(name)
    B, S, x_d = 2, 5, FLOWS[name]['x_d']
    y = _y(name, B)
    got = flow.sample(y, S, seed=6, chunk=3, return_samples=False, return_stats=False, return_y_dev=True)['y_dev']
    xy_hat = flow(_zy(name, y, S, 1.0, 6, 0), -1).cpu().numpy().astype(np.float64)
    y64 = np.repeat(_y_np(name, B).astype(np.float64), S, axis=0)
    ref = np.abs(xy_hat[..., x_d:] - y64).reshape(B * S, -1).sum(1).reshape(B, S)
    e = np.abs(got.cpu().numpy().astype(np.float64) - ref)
    print(f'{name}: y_dev worst err/bound {np.max(e / (RTOL * ref)):.3e}, sums {ref.min():.3e} .. {ref.max():.3e}')
    assert ref.min() > 0 and np.all(e <= RTOL * ref)


def _c_sample(flow, b, y, desc):
    _lib.check(_lib.load().cnf_flow_sample(flow._plan, flow.params.data_ptr(), flow._aux.data_ptr(), y.data_ptr(),
                                           C.byref(desc), b.samples.data_ptr(), b.mean.data_ptr(), b.std.data_ptr(),
                                           b.y_dev.data_ptr(), b.ws.data_ptr(), y.shape[0],
                                           torch.cuda.current_stream().cuda_stream), 'cnf_flow_sample')


def _sample_buffers(flow, pat, B, S, desc):
    H, W, D = flow.io_shape
    nbytes = int(_lib.load().cnf_plan_sample_workspace_bytes(flow._plan, B, C.byref(desc)))
    assert nbytes > 0
    return Buffers(pat, ws=nbytes, samples=(B, S, H, W, flow.x_d), mean=(B, H, W, flow.x_d), std=(B, H, W, flow.x_d),
                   y_dev=(B, S))


OUTPUTS = ('samples', 'mean', 'std', 'y_dev')


@pytest.mark.gpu
def test_sample_ignores_workspace_contents(gpu):
    """cnf_flow_sample under the fills of tests/test_state_independence.py (zeros, 0xFF, another call's
    leftovers), workspace and outputs between guard bands: bit-equal, finite, guards untouched."""
    flow, ora, P = _flow('small')
    B, S = 2, 5
    desc = _desc(S=S, chunk=3, seed=8)
    y, y_other = _y('small', B), _y('small', B, seed=11)
    res = {}
    for pat in PATTERNS:
        b = _sample_buffers(flow, pat, B, S, desc)
        if pat == 'L':
            _c_sample(flow, b, y_other, desc)
        _c_sample(flow, b, y, desc)
        res[pat] = [getattr(b, n).clone() for n in OUTPUTS]
        b.check(f'sample [{pat}]')
    assert_patterns_agree(res, OUTPUTS, 'cnf_flow_sample small B=2 S=5 chunk=3')
    ref = flow.sample(y, S, seed=8, chunk=3, return_y_dev=True)
    for n, t in zip(OUTPUTS, res['Z']):
        assert same_bits(t, ref[n]), n


@pytest.mark.gpu
def test_sample_graph_replay_equals_eager(gpu):
    """One capture of cnf_flow_sample over static buffers, two replays with y swapped in between (and every
    buffer refilled): each equals the eager call on that y."""
    flow, ora, P = _flow('small')
    B, S = 2, 5
    desc = _desc(S=S, chunk=3, seed=8)
    ys = [_y('small', B), _y('small', B, seed=11)]
    eager = [flow.sample(y, S, seed=8, chunk=3, return_y_dev=True) for y in ys]
    torch.cuda.synchronize()
    b = _sample_buffers(flow, 'Z', B, S, desc)
    y_static = ys[0].clone()
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        _c_sample(flow, b, y_static, desc)
    torch.cuda.synchronize()
    for k, y in enumerate(ys):
        with torch.cuda.stream(side):
            y_static.copy_(y)
            for n in ('ws',) + OUTPUTS:
                b.raw[n].fill_(0xFF if k else 0x00)
            graph.replay()
        b.check(f'sample replay {k}')
        for n in OUTPUTS:
            got = getattr(b, n)
            assert torch.isfinite(got).all(), (k, n)
            assert same_bits(got, eager[k][n]), f'replay {k}: {n} differs from the eager call, ' \
                                                f'max abs diff {max_diff(got, eager[k][n]):.3e}'
    del graph


@pytest.mark.gpu
def test_moments_of_the_draws(gpu):
    """With the last conv of every s,t net zeroed the flow is the identity (the oracle's known-answer test),
    so the samples are the latents: n = 64 * 64 standard normals, whose mean and variance lie within 5 sigma
    of 0 and 1 (|mean| <= 5 / sqrt(n), |var - 1| <= 5 sqrt(2 / n))."""
    flow, ora, P = _flow('tiny', 1, True)
    y = _y('tiny', 1)
    out = flow.sample(y, 64, seed=1, return_y_dev=True)
    z = out['samples'].cpu().numpy().astype(np.float64)
    n = z.size
    assert n == 64 * 64
    print(f'latent moments: mean {z.mean():+.4f} (bound {5 / np.sqrt(n):.4f}), var {z.var():.4f} '
          f'(1 +- {5 * np.sqrt(2 / n):.4f})')
    assert abs(z.mean()) <= 5 / np.sqrt(n)
    assert abs(z.var() - 1.0) <= 5 * np.sqrt(2.0 / n)
    assert float(out['y_dev'].abs().max()) == 0.0   # the identity returns y itself
