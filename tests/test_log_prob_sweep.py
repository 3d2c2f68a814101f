"""cFlow.log_prob / cnf_flow_log_prob (include/cnf.h) off the presets: the gather's four kernels, more than one
tile per image, k_logp_finish's element loop and pixel wrap, the streamed forward under append, the posterior's
dispatch edges and chosen inputs, and the logit map's domain edge against the oracle.

tests/test_flow_log_prob.py runs on tiny (8x8x2, x_d 1) and small (16x16x4, x_d 3) with NETLDS=1: k_logp_gather<1,1>
and <3,1>, one tile (HW <= 1024), at most one trip of k_logp_finish's loop, D in {2, 4}. The rows here (ROWS below;
what each reaches is asserted from the library by test_coverage_claims, through cnf_debug_logp_choice, which
reports what launch_logp_gather / launch_logp_finish themselves call):

  xy33       (8, 8, 6) x_d 3    k_logp_gather<3,3>; residual at x_d 3; D = 6 wrap in finish
  xy22       (8, 8, 4) x_d 2    k_logp_gather_any at aligned addresses, with residual
  xd1of4     (8, 8, 4) x_d 1    _any aligned, (1, 3)
  odd_d3     (16, 16, 3) x_d 2  _any (2, 1); D = 3 wrap; 768 elements (a partial only trip of finish)
  odd_d5     (8, 8, 5) x_d 3    _any (3, 2); D = 5 wrap
  min4x4     (4, 4, 2) x_d 1    4 quads, 32 elements: almost every thread idle
  w12x20     (12, 20, 4) x_d 3  60 quads, under one wave
  w2         (16, 2, 4) x_d 3   width 2
  hw1088     (32, 34, 2) x_d 1  2 tiles, 16 quads in the second; finish: two full trips and a third of 32 threads
  rect32x48  (32, 48, 4) x_d 3  2 full tiles; finish: 6 full trips; streamed by default

Each row runs on its default path; xy33, odd_d3, hw1088 and w12x20 (k_net_lds by default) also with NETLDS=0.
B = 2 images and K = 3 conditions unless stated. Weights OracleCFlow.init_params(0) ('init') and
test_flow_log_prob's 'trained'. Inputs: y standard normal; x standard normal (plain, residual) or uniform on
[0.001, 0.999] (logit: strictly inside the map's domain (-a / c1, (1 - a) / c1); the domain-edge test goes to
its ends).

Bounds. Every term against the float64 oracle under test_flow_log_prob.log_prob_reference's bounds (derived in that
file's docstring), through its check_terms; the posterior under its check_posterior. The two bounds this file adds,
written before the first GPU run:
  K = 1 posterior: lse = m + log(exp(0)) = m exactly in fp64, so posterior = (float)exp(0) = 1 exactly, and
      log_evidence = (float)(log_prob + log_prior), within one fp32 ulp at that magnitude of the float64 sum
      (check_posterior's evidence bound; its print needs a second column, so K = 1 is checked here);
  a row of -inf only: posterior NaN and log_evidence -inf, as include/cnf.h documents; such rows are taken out
      before check_posterior sees the others.
Everything else is bit equality. Measured figures: DESIGN.md (density of given images, "Off the presets")."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from arl_conditional_normalizing_flows_amd import _lib

from test_capi import _plan, schedule_of_plan
from test_flow_log_prob import (LOGIT_A, MODES, _launch_names, _pairs, _posterior_reference, _relaunch_all, _trained,
                                check_posterior, check_terms, log_prob_reference, same_bits)
from test_generative_sweep import kw_of
from test_shape_sweep import _OPTS, SWEEP, _flow, _opt_str, _oracle, _row

B_IMG, K_COND = 2, 3
_SHALLOW = ((0, 1), (1, 1), (8, 8), (2, 2))   # odd_d5's blocks
LOCAL = {
    'xy33': _row((8, 8, 6), 3, *_SHALLOW),
    'xy22': _row((8, 8, 4), 2, *_SHALLOW),
    # r4's block (no squeeze, D = 2, nk 16, cardinality 2) with R = 1. nk 8 was the intent; the planner refuses it
    # at this size ('assert not nb_channels % cardinality': 8 // dilation 8 = 1 channel for 2 groups), and
    # cardinality 1 is refused outright. The default path mixes k_net_lds with streamed layers here.
    'hw1088': _row((32, 34, 2), 1, (0,), (1,), (16,), (2,)),
}
ROWS = ['xy33', 'xy22', 'xd1of4', 'odd_d3', 'odd_d5', 'min4x4', 'w12x20', 'w2', 'hw1088', 'rect32x48']
ALSO_STREAMED = ['xy33', 'odd_d3', 'hw1088', 'w12x20']
RESIDUAL_ROWS = ['xy33', 'xy22', 'min4x4', 'hw1088']
REGIMES = ['init', 'trained']
ROW_PATHS = [(n, 'default') for n in ROWS] + [(n, 'streamed') for n in ALSO_STREAMED]
TERM_CASES = [(n, p, m) for n, p in ROW_PATHS for m in ('plain', 'logit') + (('residual',) if n in RESIDUAL_ROWS else ())]
DRAW_CASES = [(n, m) for n in ('xy33', 'odd_d5', 'hw1088') for m in ('plain', 'logit') + (('residual',) if n in RESIDUAL_ROWS else ())]
BIT_CASES = [('xy33', 'logit'), ('xy33', 'residual'), ('xy22', 'logit'), ('xy22', 'residual'), ('odd_d3', 'plain'),
             ('odd_d3', 'logit'), ('hw1088', 'logit'), ('hw1088', 'residual')]
CHUNKS = (1, 3, 5, B_IMG * K_COND, 64)
STATE_CHUNK = 4   # the schedule test's and the workspace-contents test's
EDGE_ROWS = ['tiny', 'xy33', 'hw1088']
TERMS = ('log_prob', 'llz', 'logdet', 'log_jac', 'y_dev')
ALL_KEYS = TERMS + ('posterior', 'log_evidence', 'bits_per_dim')

# LogpGatherKernel (csrc/cnf_kernels.h), cnf_debug_logp_choice's first word
ANY, T11, T31, T33 = 0, 1, 2, 3
# per row: (gather kernel at aligned addresses, tiles, finish trips, threads of the last trip holding a float4, D)
EXPECT = {
    'xy33': (T33, 1, 1, 96, 6), 'xy22': (ANY, 1, 1, 64, 4), 'xd1of4': (ANY, 1, 1, 64, 4),
    'odd_d3': (ANY, 1, 1, 192, 3), 'odd_d5': (ANY, 1, 1, 80, 5), 'min4x4': (T11, 1, 1, 8, 2),
    'w12x20': (T31, 1, 1, 240, 4), 'w2': (T31, 1, 1, 32, 4), 'hw1088': (T11, 2, 3, 32, 2),
    'rect32x48': (T31, 2, 6, 256, 4),
}


def _kw_of(name):
    """constructor arguments: a local row, or test_generative_sweep.kw_of's (presets, sweep rows)"""
    return dict(LOCAL[name], group_mode='reference') if name in LOCAL else kw_of(name)


def _capi_kw(name):
    return {k: v for k, v in _kw_of(name).items() if k != 'group_mode'}


def _chunk_ns(total, chunk):
    """the sizes n of the chunks of one call"""
    return {min(chunk, total)} | ({total % chunk} if total % chunk else set())


def _choice(lib, p, n, aligned=1):
    w = (C.c_int * 6)()
    assert lib.cnf_debug_logp_choice(p, n, aligned, w, 6) == 6
    return list(w)


class _Plan:
    def __init__(self, lib, name, options=None):
        self.lib = lib
        rc, self.p, self.keep = _plan(lib, _capi_kw(name), options=_opt_str(options))
        assert rc == 0, (name, lib.cnf_last_error())

    def __enter__(self):
        return self.p

    def __exit__(self, *exc):
        self.lib.cnf_plan_destroy(self.p)


@functools.lru_cache(maxsize=None)
def _model(name, regime='init'):
    """(kw, oracle, weights) of a row or preset; the sweep rows share test_shape_sweep._oracle's cache"""
    from oracle.cflow_np import OracleCFlow
    if name in SWEEP:
        kw, ora, P = _oracle(name)[:3]
    else:
        kw = _kw_of(name)
        ora = OracleCFlow(**kw)
        P = ora.init_params(0)
    if regime == 'trained':
        P = _trained(ora.init_params(2))
    return kw, ora, P


@functools.lru_cache(maxsize=None)
def _inputs(name, mode, B=B_IMG, K=K_COND):
    """fp32 (x [B,H,W,x_d] in sample space, y [K,H,W,D-x_d]), left unchanged"""
    kw = _kw_of(name)
    H, W, D = kw['io_shape']
    x_d = kw['x_d']
    rng = np.random.default_rng(41)
    y = rng.standard_normal((K, H, W, D - x_d)).astype(np.float32)
    if mode == 'logit':
        x = rng.uniform(0.001, 0.999, (B, H, W, x_d)).astype(np.float32)
    else:
        x = rng.standard_normal((B, H, W, x_d)).astype(np.float32)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def _in_domain(x, a=LOGIT_A):
    """strictly inside the logit map's domain in exact arithmetic: 0 < a + (1 - 2 a) x < 1"""
    e = a + (1.0 - 2.0 * a) * np.asarray(x, np.float64)
    return (e > 0.0) & (e < 1.0)


@functools.lru_cache(maxsize=None)
def _reference(name, mode, regime):
    """float64 (ref, tol) of the B K expanded pairs of _inputs, computed once per case"""
    kw, ora, P = _model(name, regime)
    x, y = _inputs(name, mode)
    with np.errstate(over='ignore', invalid='ignore'):
        return log_prob_reference(ora, P, *_pairs(x, y), **MODES[mode])


# ---------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------

def test_coverage_claims(lib):
    """What the docstring says the rows reach, from the host functions the launches call (cnf_debug_logp_choice): a
    change of a row, of launch_logp_gather's choice or of LOGP_QUADS fails here instead of silently emptying the
    GPU part."""
    assert sorted(EXPECT) == sorted(ROWS)
    seen_np, per_row = set(), {}
    for name in ROWS:
        kw = _kw_of(name)
        H, W, D = kw['io_shape']
        ns = set().union(*[_chunk_ns(B_IMG * K_COND, c) for c in CHUNKS + (STATE_CHUNK,)])
        with _Plan(lib, name) as p:
            w = _choice(lib, p, B_IMG * K_COND)
            per_row[name] = (w[0], w[1], w[4], w[5], D)
            assert _choice(lib, p, B_IMG * K_COND, aligned=0)[0] == ANY, name
            for n in sorted(ns):
                kernel, parts, per_xcd, grid, trips, last = _choice(lib, p, n)
                assert (kernel, parts, trips, last) == (w[0], w[1], w[4], w[5])   # (the image shape alone)
                # every item has a workgroup and fewer than 8 workgroups are spare
                assert grid == 8 * per_xcd and 0 <= grid - n * parts < 8, (name, n, grid)
                if name in ('hw1088', 'xy33', 'xy22', 'odd_d3'):   # the rows of the chunk tests
                    seen_np.add(n * parts)
            fwd = schedule_of_plan(lib, p, B_IMG * K_COND, 1)
        lds = [s for s in fwd if s == 'k_net_lds']
        if name in ALSO_STREAMED:   # k_net_lds by default, so NETLDS=0 is another path
            assert lds, (name, fwd)
            with _Plan(lib, name, _OPTS['streamed']) as p:
                assert 'k_net_lds' not in schedule_of_plan(lib, p, B_IMG * K_COND, 1), name
    print('row: (kernel, parts, finish trips, last trip threads, D)', per_row)
    assert per_row == EXPECT
    assert {k for k, *_ in per_row.values()} == {ANY, T11, T31, T33}
    assert {v[1] for v in per_row.values()} == {1, 2}
    assert per_row['hw1088'][2:4] == (3, 32) and per_row['rect32x48'][2] >= 6 and per_row['odd_d3'][2] == 1
    assert {v[4] for v in per_row.values()} == {2, 3, 4, 5, 6}
    # the tile-major item mapping: fewer items than XCDs, exactly 8, and more with a remainder
    print('n * parts on the chunk rows:', sorted(seen_np))
    assert any(v < 8 for v in seen_np) and 8 in seen_np and any(v > 8 and v % 8 for v in seen_np)
    assert {2, 6, 10, 12} <= seen_np   # (hw1088 under CHUNKS)
    # rect32x48 streams by default: some coupling runs outside k_net_lds
    with _Plan(lib, 'rect32x48') as p:
        fwd = schedule_of_plan(lib, p, B_IMG * K_COND, 1)
        assert any(s.startswith('k_pw') for s in fwd), fwd
    # the element-by-element gather's residual branch runs where x_d == D - x_d and no template exists
    assert EXPECT['xy22'][0] == ANY and 'xy22' in RESIDUAL_ROWS
    # the posterior's dispatch edge (launch_logp_posterior: one wave per row up to 64 conditions)
    assert {63, 64, 65} <= {K for _, K in POSTERIOR_SHAPES} and max(K for _, K in POSTERIOR_SHAPES) > 2 * 256


@pytest.mark.parametrize('name', ['hw1088', 'rect32x48'])
def test_workspace_with_two_tiles(lib, name):
    """test_flow_log_prob.test_workspace_does_not_scale_with_pairs's formula at parts = 2 (the library's count):
    the forward workspace of one chunk plus one chunk each of xy, zy, the log-det and two log_jac slots per pair,
    whatever B and K."""
    H, W, D = _kw_of(name)['io_shape']
    with _Plan(lib, name) as p:
        parts = _choice(lib, p, 1)[1]
        assert parts == 2
        for chunk in (1, 7, 64):
            need = int(lib.cnf_plan_workspace_bytes(p, chunk)) + chunk * (2 * H * W * D * 4 + 4 + 8 * parts)
            got = {(B, K): int(lib.cnf_plan_logp_workspace_bytes(p, B, C.byref(_lib.cnf_logp_desc(K, chunk, 0.0, 0))))
                   for B in (1, 1000) for K in (0, 1, 10, 1000)}
            assert len(set(got.values())) == 1, got
            assert need <= got[(1, 0)] <= need + 5 * 256, (name, chunk, got[(1, 0)], need)


@pytest.mark.parametrize('name', ROWS)
def test_references_are_usable(name):
    """For every (row, mode, regime) of the GPU part: the float64 terms and bounds are finite, the bounds positive
    where the term is not identically 0, and with the logit map every x element lies strictly inside the domain."""
    for mode in ('plain', 'logit') + (('residual',) if name in RESIDUAL_ROWS else ()):
        x, y = _inputs(name, mode)
        if mode == 'logit':
            assert _in_domain(x).all() and 0.0 < float(x.min()) and float(x.max()) < 1.0
        for regime in REGIMES:
            ref, tol = _reference(name, mode, regime)
            for k in TERMS:
                assert ref[k].shape == (B_IMG * K_COND,) and np.isfinite(ref[k]).all() and np.isfinite(tol[k]).all(), \
                    (name, mode, regime, k, ref[k])
                assert k == 'log_jac' and mode != 'logit' or (tol[k] > 0).all(), (name, mode, regime, k)
            print(f'{name} {mode} {regime}: |log_prob| <= {np.abs(ref["log_prob"]).max():.3e}, '
                  f'|llz| <= {np.abs(ref["llz"]).max():.3e}')


def _edge_spots(name):
    """(index, value) of the domain-edge test: x exactly 0 and 1 and their fp32 neighbours inside (0, 1), in both
    images, first and last pixels (hw1088: pixels >= 1024, the second tile) and first and last x channel"""
    kw = _kw_of(name)
    H, W, _ = kw['io_shape']
    c = kw['x_d'] - 1
    lo, hi = np.float32(0.0), np.float32(1.0)
    return [((0, 0, 0, 0), lo), ((0, 1, 2, c), hi), ((0, H - 1, W - 1, 0), np.nextafter(lo, hi)),
            ((0, H - 1, 3, c), np.nextafter(hi, lo)), ((0, H - 1, 2, 0), hi), ((1, H - 1, W - 2, c), lo),
            ((1, 0, 1, 0), np.nextafter(hi, lo)), ((1, 2, 0, c), np.nextafter(lo, hi)), ((1, H - 1, 0, 0), hi)]


@functools.lru_cache(maxsize=None)
def _edge_inputs(name):
    x, y = _inputs(name, 'logit')
    x = x.copy()
    for idx, v in _edge_spots(name):
        x[idx] = v
    x.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def _edge_reference(name):
    kw, ora, P = _model(name)
    return log_prob_reference(ora, P, *_pairs(*_edge_inputs(name)), logit_a=LOGIT_A)


@pytest.mark.parametrize('name', EDGE_ROWS)
def test_edge_reference_supports_fp32_e(name):
    """Before the GPU sees the domain-edge inputs: the kernel's own arithmetic, emulated in numpy (e = fmaf(c1, x, a)
    rounded to fp32 from the fp32 constants of logit_consts, then -log(e (1 - e)) in float64 plus the shared
    constant), stays within the log_jac bound of the float64 reference on these x. The edge values are x = 0, 1 and
    their fp32 neighbours 1.4e-45 and 1 - 2^-24; at 1 - 2^-24 the fp32 e = 0.99 carries half an ulp (3e-8) against
    1 - e = 0.01, 3e-6 of that element's term, against a bound of 1e-5 of the image's sum of |terms| (printed): no
    element had to be moved inwards."""
    x, y = _edge_inputs(name)
    assert _in_domain(x).all()
    assert {float(v) for _, v in _edge_spots(name)} == {0.0, 1.0, float(np.nextafter(np.float32(0), np.float32(1))),
                                                        float(np.nextafter(np.float32(1), np.float32(0)))}
    ref, tol = _edge_reference(name)
    assert all(np.isfinite(ref[k]).all() for k in TERMS)
    ad = float(np.float32(LOGIT_A))
    c1 = np.float32((1.0 - ad) * ((1.0 - 2.0 * ad) / (1.0 - ad)))
    span = np.log(np.float32((1.0 - ad) / ad)) - np.log(np.float32(ad / (1.0 - ad)))   # (fp32 logs, as logit_consts)
    assert span.dtype == np.float32
    e = (np.float64(c1) * x.astype(np.float64) + ad).astype(np.float32).astype(np.float64)
    assert ((e > 0) & (e < 1)).all()
    n_el = x[0].size
    lj = (-np.log(e * (1.0 - e))).reshape(len(x), -1).sum(1) + n_el * (np.log(np.float64(c1)) - np.log(np.float64(span)))
    want, bound = ref['log_jac'][::K_COND], tol['log_jac'][::K_COND]   # (pair b K is image b)
    print(f'{name}: fp32-e log_jac off the float64 one by {np.abs(lj - want)} of a bound {bound} '
          f'(margin x{np.min(bound / np.maximum(np.abs(lj - want), 1e-300)):.1f})')
    assert np.all(np.abs(lj - want) <= bound)


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _gpu_flow(gpu, name, path='default', regime='init'):
    kw, ora, P = _model(name, regime)
    return _flow(kw, P, gpu, _OPTS[path])


def _t(a, gpu):
    return torch.tensor(np.asarray(a), device=gpu)   # (a copy: the cached inputs are read-only)


@pytest.mark.gpu
@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('name,path,mode', TERM_CASES)
def test_terms_match_oracle(gpu, name, path, mode, regime):
    """Every term of the pairwise call (2 images x 3 conditions, one chunk of 6) against the float64 oracle under
    test_flow_log_prob's bounds. check_terms prints each term's worst err/tol; DESIGN.md has the sweep's maxima."""
    flow = _gpu_flow(gpu, name, path, regime)
    x, y = _inputs(name, mode)
    out = flow.log_prob(_t(x, gpu), _t(y, gpu), pairwise=True, return_terms=True, **MODES[mode])
    assert all(out[k].shape == (B_IMG, K_COND) for k in TERMS)
    if mode != 'logit':
        assert float(out['log_jac'].abs().max()) == 0.0
    ref, tol = _reference(name, mode, regime)
    check_terms(out, ref, tol, f'{name} {path} {mode} {regime}')


@pytest.mark.gpu
@pytest.mark.parametrize('name,mode', DRAW_CASES)
def test_own_draws_match_oracle(gpu, name, mode):
    """test_flow_log_prob.test_own_draws_match_oracle on the rows: x = the model's own draws, each under the
    condition it was drawn for. With the logit map the draws are taken at temperature 0.1, for the reason given
    there: at temperature 1 the untrained flow draws values that the fp32 de_logitify returns as the domain's edge
    exactly (density -inf by definition) or squeezes into a few ulp of the other edge, where an fp32 x no longer
    pins down log(e) to 1e-5. Printed, not asserted: log_prob - log_jac - sample's log_prob (see there)."""
    kw, ora, P = _model(name)
    flow = _gpu_flow(gpu, name)
    S = K_COND
    y = _t(_inputs(name, mode)[1][:B_IMG], gpu)
    drawn = flow.sample(y, S, temperature=0.1 if mode == 'logit' else 1.0, seed=3, return_stats=False,
                        return_log_prob=True, **MODES[mode])
    x = drawn['samples'].reshape((B_IMG * S,) + tuple(drawn['samples'].shape[2:])).contiguous()
    yy = y.repeat_interleave(S, dim=0).contiguous()
    out = flow.log_prob(x, yy, return_terms=True, **MODES[mode])
    assert out['log_prob'].shape == (B_IMG * S,)
    if mode == 'logit':
        assert _in_domain(x.cpu().numpy()).all()
    ref, tol = log_prob_reference(ora, P, x.cpu().numpy(), yy.cpu().numpy(), **MODES[mode])
    check_terms(out, ref, tol, f'{name} {mode} own draws')
    d = (out['log_prob'].double() - out['log_jac'].double() - drawn['log_prob'].reshape(-1).double()).abs()
    print(f'{name} {mode}: worst |log_prob - log_jac - sample log_prob| {float(d.max()):.3e} '
          f'(|log_prob| <= {float(out["log_prob"].abs().max()):.3e})')


def _offset4(t):
    """the same values at an address 4 bytes past a 16-byte boundary"""
    o = torch.empty(t.numel() + 1, device=t.device)[1:].view(t.shape).copy_(t)
    assert o.data_ptr() % 16 == 4 and o.is_contiguous()
    return o


@pytest.mark.gpu
@pytest.mark.parametrize('name,mode', BIT_CASES)
def test_pairwise_equals_paired_and_unaligned(gpu, name, mode):
    """[B,K] of one pairwise call == the paired call on the B K expanded pairs == the pairwise call on x and y at
    addresses 4 bytes off a 16-byte boundary, bit for bit, every term. At aligned addresses xy33 and hw1088 run a
    template and the unaligned call k_logp_gather_any; xy22 and odd_d3 run _any both times."""
    flow = _gpu_flow(gpu, name)
    x, y = (_t(a, gpu) for a in _inputs(name, mode))
    assert x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0
    kw = dict(return_terms=True, **MODES[mode])
    pw = flow.log_prob(x, y, pairwise=True, **kw)
    pd = flow.log_prob(*(_t(a, gpu) for a in _pairs(*_inputs(name, mode))), **kw)
    off = flow.log_prob(_offset4(x), _offset4(y), pairwise=True, **kw)
    for k in TERMS + ('bits_per_dim',):
        assert torch.isfinite(pw[k]).all()
        assert same_bits(pw[k].reshape(-1), pd[k]), f'{name} {mode}: {k} differs between pairwise and paired'
        assert same_bits(pw[k], off[k]), f'{name} {mode}: {k} differs at an unaligned address'
    assert (pw['log_prob'].max(dim=1).values > pw['log_prob'].min(dim=1).values).all()


@pytest.mark.gpu
@pytest.mark.parametrize('name,mode', BIT_CASES)
def test_no_dependence_on_chunk(gpu, name, mode):
    """chunk in {1, 3, 5, B K, 64}, chunks straddling images: every term and the posterior bit-equal. On hw1088 the
    gather's grids hold 2, 6, 10 and 12 items (n * parts), so the tile-major mapping and its XCD remap run with
    fewer items than XCDs and with a remainder."""
    flow = _gpu_flow(gpu, name)
    x, y = (_t(a, gpu) for a in _inputs(name, mode))
    ref = None
    for chunk in CHUNKS:
        got = flow.log_prob(x, y, pairwise=True, chunk=chunk, return_terms=True, return_posterior=True, **MODES[mode])
        assert sorted(got) == sorted(ALL_KEYS)
        ref = got if ref is None else ref
        for k in ALL_KEYS:
            assert same_bits(got[k], ref[k]), f'{name} {mode} chunk={chunk}: {k} differs'
    assert torch.isfinite(ref['log_prob']).all()
    assert (ref['log_prob'].max(dim=1).values > ref['log_prob'].min(dim=1).values).all()


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['logit', 'residual'])
def test_schedule_and_no_dependence_on_workspace(gpu, mode):
    """hw1088 with chunk 4 (chunks of 4 and 2 pairs, 8 and 4 gather items). The recording holds, per chunk,
    k_logp_gather, the forward's launches at that chunk's own n (cnf_debug_schedule, direction +1) and
    k_logp_finish, then k_logp_posterior. The same bits after the workspace, whose lj slots have two columns here,
    was filled with 0xFF bytes (every float and double a NaN), and from a relaunch of the recording into NaN-filled
    outputs over a NaN-filled workspace."""
    name = 'hw1088'
    lib = _lib.load()
    flow = _gpu_flow(gpu, name)
    x, y = (_t(a, gpu) for a in _inputs(name, mode))
    kw = dict(pairwise=True, chunk=STATE_CHUNK, return_terms=True, return_posterior=True, **MODES[mode])
    ref = {k: v.clone() for k, v in flow.log_prob(x, y, **kw).items()}
    assert all(torch.isfinite(ref[k]).all() for k in ALL_KEYS)
    ws = flow._ws[('log_prob', STATE_CHUNK)]
    ws.fill_(0xFF)
    out = flow.log_prob(x, y, **kw)
    for k in ALL_KEYS:
        assert same_bits(out[k], ref[k]), f'{name} {mode} NaN workspace: {k} differs'
    names = _launch_names(flow)
    with _Plan(lib, name) as p:
        fwd = {n: schedule_of_plan(lib, p, n, 1) for n in (4, 2)}
    want = []
    for n in (4, 2):
        want += ['k_logp_gather'] + fwd[n] + ['k_logp_finish']
    assert names == want + ['k_logp_posterior'], names
    torch.cuda.synchronize()
    ws.fill_(0xFF)
    for k in ALL_KEYS:
        if k != 'bits_per_dim':   # (computed by torch from log_prob, not a launch)
            out[k].fill_(float('nan'))
    assert _relaunch_all(flow, torch.cuda.current_stream().cuda_stream) == len(names)
    torch.cuda.synchronize()
    for k in ALL_KEYS:
        if k != 'bits_per_dim':
            assert same_bits(out[k], ref[k]), f'{name} {mode} relaunch: {k} differs'


@pytest.mark.gpu
@pytest.mark.parametrize('name', EDGE_ROWS)
def test_domain_edge_matches_oracle(gpu, name):
    """logit_a = 0.01 with x elements exactly 0 and 1 and at their fp32 neighbours inside (0, 1) (_edge_spots; the
    CPU test test_edge_reference_supports_fp32_e shows the float64 reference supports the bound there): every term
    against the oracle under the unchanged bounds. Then one element outside the domain (above, below, NaN) in image
    1, on hw1088 at pixel 31 * 34 + 5 = 1059 >= 1024, the second tile: that image's pairs get -inf, image 0 keeps
    its bits."""
    flow = _gpu_flow(gpu, name)
    xn, yn = _edge_inputs(name)
    x, y = _t(xn, gpu), _t(yn, gpu)
    kw = dict(pairwise=True, return_terms=True, return_posterior=True, logit_a=LOGIT_A)
    ref = flow.log_prob(x, y, **kw)
    check_terms(ref, *_edge_reference(name), f'{name} domain edge')
    H, W, _ = _kw_of(name)['io_shape']
    spot = (1, H - 1, 5, 0)
    assert spot not in [i for i, _ in _edge_spots(name)] and (name != 'hw1088' or (H - 1) * W + 5 >= 1024)
    for value in (1.02, -0.02, float('nan')):
        bad = x.clone()
        bad[spot] = value
        got = flow.log_prob(bad, y, **kw)
        assert torch.isneginf(got['log_prob'][1]).all() and torch.isneginf(got['log_jac'][1]).all(), value
        assert torch.isposinf(got['bits_per_dim'][1]).all()
        assert torch.isnan(got['posterior'][1]).all() and float(got['log_evidence'][1]) == float('-inf')
        for k in ('llz', 'logdet', 'y_dev'):
            assert torch.isnan(got[k][1]).all(), (value, k)
        for k in ALL_KEYS:
            assert same_bits(got[k][0], ref[k][0]), f'{name} x={value}: {k} of image 0 changed'


# (B, K): one pair; a partly filled second workgroup of the wave form (B = 5); the dispatch edge 63 / 64 / 65; the
# workgroup form's one full trip (256), its second trip of one entry (257) and a third trip (600)
POSTERIOR_SHAPES = [(1, 1), (5, 2), (4, 63), (5, 64), (5, 65), (2, 256), (3, 257), (2, 600)]


def _posterior_call(gpu, B, K):
    flow = _gpu_flow(gpu, 'min4x4')
    kw = _kw_of('min4x4')
    H, W, D = kw['io_shape']
    rng = np.random.default_rng(1000 * B + K)
    x = _t(rng.standard_normal((B, H, W, kw['x_d'])).astype(np.float32), gpu)
    y = _t(rng.standard_normal((K, H, W, D - kw['x_d'])).astype(np.float32), gpu)
    prior = torch.linspace(-3.0, 3.0, K, device=gpu) if K > 1 else torch.full((1,), -3.0, device=gpu)
    return flow, prior, flow.log_prob(x, y, pairwise=True, log_prior=prior)


def _check_posterior_rows(out, prior, what):
    """check_posterior on the rows some condition explains; a row of -inf only has a NaN posterior and -inf
    evidence; K = 1: the posterior is exactly 1 (module docstring)"""
    B, K = out['log_prob'].shape
    a = _posterior_reference(out['log_prob'], prior)[2]
    none = torch.isneginf(a).all(dim=1)
    assert torch.isnan(out['posterior'][none]).all() and torch.isneginf(out['log_evidence'][none]).all(), what
    keep = ~none
    assert not torch.isnan(out['posterior'][keep]).any()
    if not keep.any():
        return
    if K == 1:
        assert torch.equal(out['posterior'][keep], torch.ones_like(out['posterior'][keep])), what
        a1 = a[keep, 0].cpu().numpy()
        e = np.abs(out['log_evidence'][keep].double().cpu().numpy() - a1)
        print(f'{what}: posterior exactly 1, worst log_evidence err {e.max():.3e}')
        assert np.all(e <= np.spacing(np.abs(a1).astype(np.float32)).astype(np.float64)), (e, a1)
        return
    check_posterior({k: out[k][keep] for k in ('log_prob', 'posterior', 'log_evidence')}, prior, what)


@pytest.mark.gpu
@pytest.mark.parametrize('B,K', POSTERIOR_SHAPES)
def test_posterior_shapes(gpu, B, K):
    """Real calls on min4x4 with a non-uniform prior: both forms of k_logp_posterior at their edges, under
    check_posterior's bounds."""
    flow, prior, out = _posterior_call(gpu, B, K)
    assert out['posterior'].shape == (B, K) and out['log_evidence'].shape == (B,)
    assert torch.isfinite(out['log_prob']).all()
    _check_posterior_rows(out, prior, f'min4x4 B={B} K={K}')


def _crafted_rows(K, gpu):
    """chosen rows of log_prob [.., K]: ties, a spread of +-5000 nats, -inf among finite entries, -inf only, the
    maximum in the last column (column 256 at K = 257: the one entry of the workgroup form's second trip), and a
    row whose maximum is -3e38"""
    g = torch.Generator().manual_seed(K)
    ninf = float('-inf')
    ties = torch.full((K,), -123.25)
    spread = torch.linspace(-5000.0, 5000.0, K)[torch.randperm(K, generator=g)]
    one = torch.full((K,), ninf)
    one[K // 3] = -77.5
    none = torch.full((K,), ninf)
    last = torch.randn(K, generator=g) * 3.0 - 50.0
    last[K - 1] = -20.0
    huge = torch.full((K,), -3.4e38)
    huge[K // 2] = -3e38
    huge[K - 2] = ninf
    mixed = torch.randn(K, generator=g) * 2.0
    mixed[::3] = ninf
    return torch.stack([ties, spread, one, none, last, huge, mixed]).to(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize('K', [64, 65, 257])
def test_posterior_on_chosen_rows(gpu, K):
    """k_logp_posterior alone on chosen inputs: after one real call (B = 5) the returned log_prob tensor is
    overwritten in place and the last recorded launch, k_logp_posterior, is relaunched into NaN-filled outputs;
    against _posterior_reference under check_posterior's bounds. With and without the -inf rows' neighbours being
    finite, so a row cannot borrow another's maximum or sum."""
    B = 5
    lib = _lib.load()
    flow, prior, out = _posterior_call(gpu, B, K)
    names = _launch_names(flow)
    assert names[-1] == 'k_logp_posterior' and names.count('k_logp_posterior') == 1
    rows = _crafted_rows(K, gpu)
    assert float((rows[4] + prior).argmax()) == K - 1   # the maximum in the last column with the prior too
    assert float(rows[5].max()) == float(torch.tensor(-3e38)) and torch.isneginf(rows[3]).all()
    stream = torch.cuda.current_stream().cuda_stream
    for pick in ([0, 1, 2, 3, 4], [5, 6, 3, 3, 1], [3, 3, 3, 3, 3]):
        torch.cuda.synchronize()
        out['log_prob'].copy_(rows[pick])
        out['posterior'].fill_(float('nan'))
        out['log_evidence'].fill_(float('nan'))
        _lib.check(lib.cnf_plan_relaunch(flow._plan, len(names) - 1, stream), 'cnf_plan_relaunch')
        torch.cuda.synchronize()
        assert same_bits(out['log_prob'], rows[pick])   # (an input of the launch: untouched)
        _check_posterior_rows(out, prior, f'K={K} rows {pick}')
        assert not torch.isnan(out['log_evidence']).any()
        if 0 in pick:   # ties: the posterior is the prior's softmax
            want = torch.softmax(prior.double(), 0)
            assert float((out['posterior'][pick.index(0)].double() - want).abs().max()) <= 4 * K * 2.0 ** -23
        if 2 in pick:   # one finite entry: it takes everything, exactly
            r = out['posterior'][pick.index(2)]
            assert float(r[K // 3]) == 1.0 and float(r.sum()) == 1.0
