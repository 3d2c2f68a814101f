"""Cascaded super-resolution sampling: cnf_flow_sample_cascade / cFlowCascade.sample (include/cnf.h): L flows
chained, each stage's draws `up`-scaled into the next stage's conditions, walked depth-first one chunk per stage.

CPU part (host only, placeholder addresses): every argument error is CNF_E_INVALID with a message naming the
argument (and the stage) before any HIP call; a valid one-stage call gets as far as cnf_flow_sample; the workspace
is the sum of the stages' sample workspaces, whatever the S_l; cFlowCascade refuses a broken chain.

GPU part: the cascade equals the composition of the public calls (cFlow.sample -> base_functions.up -> cFlow.sample
...) bit for bit, so its correctness against the float64 oracle is the existing sampling tests'; no output depends on
chunk, on what the buffers held, or on which other outputs are requested, bit for bit; per-stage mean / std within
test_sampling.stats_bounds of the float64 statistics of that stage's samples; rank and hist integer-equal to numpy,
abs_err / sq_err / quantiles within test_sample_score's bounds with S = N_L; block_dev within block_dev_bound below
(written before the first GPU run); the structural cases (temperature 0, identity flows).

Flows: x_d 1: the shape-sweep row 'min4x4' (4x4x2) -> preset 'tiny' (8x8x2) -> a 16x16x2 flow; x_d 3, not square:
6x10x6 -> 12x20x6 (720 elements per leaf condition: 22 fold tiles and a half; D = 6: the element form of
k_child_latent, as D = 2); x_d 2: 8x8x4 -> 16x16x4 (D = 4: the 16-byte form, a quad holding two x and two y
channels). Weights OracleCFlow.init_params(stage + 1); y_1 = up of a seeded uniform low-resolution batch."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from arl_conditional_normalizing_flows_amd import _lib
from arl_conditional_normalizing_flows_amd.config import PRESETS
from oracle.cflow_np import OracleCFlow

from test_capi import _plan
from test_sample_score import SQ_RTOL, _np_rank_hist, _score_desc, abs_err_bound, quantile_bounds
from test_sampling import A, OUT, WS, U, Y, _desc, stats_bounds
from test_shape_sweep import SWEEP
from test_state_independence import PATTERNS, Buffers, same_bits


def _row(shape, x_d, sq, rx, nk, card):
    return dict(io_shape=shape, x_d=x_d, squeeze_factor_block_list=sq, ResNeXt_block_list=rx, num_kernels_list=nk,
                cardinality_list=card, group_mode='reference')


FLOWS = {
    's4': dict(SWEEP['min4x4'], group_mode='reference'),
    's8': PRESETS['tiny'].kwargs(),
    's16': _row((16, 16, 2), 1, (0, 1), (1, 1), (16, 16), (2, 2)),
    'r6x10': _row((6, 10, 6), 3, (0, 1), (1, 1), (8, 8), (2, 2)),
    'r12x20': _row((12, 20, 6), 3, (0, 1), (1, 1), (8, 8), (2, 2)),
    'v8': _row((8, 8, 4), 2, (0, 1), (1, 1), (8, 8), (2, 2)),
    'v16': _row((16, 16, 4), 2, (0, 1), (1, 1), (8, 8), (2, 2)),
    'small': PRESETS['small'].kwargs(),   # 16x16x4, x_d 3: io_d != 2 x_d
}
CHAINS = {'x1': ('s4', 's8'), 'x1L3': ('s4', 's8', 's16'), 'x3': ('r6x10', 'r12x20'), 'x2': ('v8', 'v16'), 'one': ('s8',)}
LEVELS = (0.05, 0.5, 0.95)
BINS = 16


def _capi_kw(name):
    return {k: v for k, v in FLOWS[name].items() if k != 'group_mode'}


# ---------------------------------------------------------------------------------------------
# CPU: the C ABI's host side
# ---------------------------------------------------------------------------------------------

def _cdesc(L=2, S=(3, 4), chunk=3, T=1.0, seed=0, offset=0, logit_a=0.0, residual=0):
    d = _lib.cnf_cascade_desc()
    d.num_stages, d.chunk, d.seed, d.logit_a, d.residual = L, chunk, seed, logit_a, residual
    for l in range(min(max(L, 0), 4)):
        d.num_samples[l] = S[l] if l < len(S) else 1
        d.temperature[l] = T[l] if isinstance(T, tuple) else T
        d.offset[l] = offset
    return d


class _Plans:
    """the plans of a chain, created on the host and destroyed on exit"""

    def __init__(self, lib, names):
        self.lib, self.names, self.plans, self.keep = lib, names, [], []

    def __enter__(self):
        for n in self.names:
            rc, p, keep = _plan(self.lib, _capi_kw(n))
            assert rc == 0, (n, self.lib.cnf_last_error())
            self.plans.append(p)
            self.keep.append(keep)
        return self.plans

    def __exit__(self, *exc):
        for p in self.plans:
            self.lib.cnf_plan_destroy(p)


def _arr(vals):
    return (C.c_void_p * len(vals))(*vals)


_NAMES = ('plans', 'params', 'aux', 'y', 'desc', 'score', 'truth', 'samples', 'rank', 'abs_err', 'sq_err', 'hist',
          'quantiles', 'mean', 'std', 'y_dev', 'block_dev', 'ws', 'B')


def _call(lib, chain_plans, **over):
    """cnf_flow_sample_cascade on placeholder addresses: by default every output of every stage"""
    L = len(chain_plans)
    per = lambda k: _arr([OUT + ((16 + 4 * k + l) << 30) for l in range(L)])
    a = dict(plans=_arr([p.value for p in chain_plans]), params=_arr([A] * L), aux=_arr([A] * L), y=Y, desc=_cdesc(L=L),
             score=_score_desc(), truth=OUT + (8 << 30), samples=OUT, rank=OUT + (9 << 30), abs_err=OUT + (10 << 30),
             sq_err=OUT + (11 << 30), hist=OUT + (12 << 30), quantiles=OUT + (13 << 30), mean=per(0), std=per(1),
             y_dev=per(2), block_dev=per(3), ws=WS, B=2)
    assert set(over) <= set(a), over
    a.update(over)
    for k in ('desc', 'score'):
        a[k] = None if a[k] is None else C.byref(a[k])
    return lib.cnf_flow_sample_cascade(*[a[n] for n in _NAMES], None)


_NO_SCORES = dict(score=None, truth=None, rank=None, abs_err=None, sq_err=None, hist=None, quantiles=None)
_NO_OUTPUT = dict(_NO_SCORES, samples=None, mean=None, std=None, y_dev=None, block_dev=None)
_NULL2 = lambda: _arr([None, None])

# (id, chain, overrides of _call (callables are called with the plans), words the message holds)
ARG_ERRORS = [
    ('null_desc', 'x1', dict(desc=None), ('descriptor',)),
    ('stages0', 'x1', dict(desc=_cdesc(L=0)), ('num_stages',)),
    ('stages5', 'x1', dict(desc=_cdesc(L=5)), ('num_stages',)),
    ('null_plans', 'x1', dict(plans=None), ('plans',)),
    ('null_params', 'x1', dict(params=None), ('params',)),
    ('null_aux', 'x1', dict(aux=None), ('aux',)),
    ('null_plan_entry', 'x1', dict(plans=lambda p: _arr([p[0].value, None])), ('stage 2', 'plan')),
    ('null_params_entry', 'x1', dict(params=_arr([A, None])), ('stage 2', 'params')),
    ('null_aux_entry', 'x1', dict(aux=_arr([None, A])), ('stage 1', 'aux')),
    ('null_y', 'x1', dict(y=None), ('y',)),
    ('null_ws', 'x1', dict(ws=None), ('workspace',)),
    ('B0', 'x1', dict(B=0), ('B',)),
    ('S0_stage1', 'x1', dict(desc=_cdesc(S=(0, 4))), ('num_samples',)),
    ('S0_stage2', 'x1', dict(desc=_cdesc(S=(3, 0))), ('stage 2', 'num_samples')),
    ('S_negative_stage3', 'x1L3', dict(desc=_cdesc(L=3, S=(3, 2, -1))), ('stage 3', 'num_samples')),
    ('N_overflow', 'x1', dict(desc=_cdesc(S=(65536, 32768))), ('num_samples', 'stage 2')),
    ('chunk0', 'x1', dict(desc=_cdesc(chunk=0)), ('chunk',)),
    ('T_negative_stage2', 'x1', dict(desc=_cdesc(T=(1.0, -0.5))), ('stage 2', 'temperature')),
    ('T_nan', 'x1', dict(desc=_cdesc(T=float('nan'))), ('temperature',)),
    ('T_inf_stage2', 'x1', dict(desc=_cdesc(T=(0.0, float('inf')))), ('stage 2', 'temperature')),
    ('logit_half', 'x1', dict(desc=_cdesc(logit_a=0.5)), ('logit_a',)),
    ('logit_negative', 'x1', dict(desc=_cdesc(logit_a=-0.01)), ('logit_a',)),
    ('x_d_mismatch', ('s4', 'v8'), {}, ('stage 2', 'x_d')),
    ('shape_mismatch', ('s4', 's16'), {}, ('stage 2', 'io shape')),
    ('shape_mismatch_stage3', ('s4', 's8', 's8'), dict(desc=_cdesc(L=3, S=(2, 2, 2))), ('stage 3', 'io shape')),
    ('shape_not_twice', ('r6x10', 'v16'), {}, ('stage 2',)),
    ('io_d_not_2x_d', ('small',), dict(desc=_cdesc(L=1)), ('stage 1', 'io_d')),
    ('no_output', 'x1', _NO_OUTPUT, ('output',)),
    ('no_output_null_entries', 'x1', dict(_NO_OUTPUT, mean=_NULL2(), std=_NULL2(), y_dev=_NULL2(), block_dev=_NULL2()),
     ('output',)),
    ('rank_without_truth', 'x1', dict(truth=None), ('truth',)),
    ('hist_bins0', 'x1', dict(score=_score_desc(bins=0)), ('bins',)),
    ('bins257', 'x1', dict(score=_score_desc(bins=257)), ('bins',)),
    ('lo_above_hi', 'x1', dict(score=_score_desc(lo=2.0, hi=-2.0)), ('hi',)),
    ('quantiles_without_hist', 'x1', dict(hist=None), ('hist',)),
    ('num_quantiles9', 'x1', dict(score=_score_desc(levels=(0.5,) * 9)), ('num_quantiles',)),
    ('level_above_1', 'x1', dict(score=_score_desc(levels=(0.5, 1.5))), ('quantiles',)),
    ('null_score_descriptor', 'x1', dict(score=None), ('score descriptor',)),
]


@pytest.mark.parametrize('case,chain,over,words', ARG_ERRORS, ids=[c[0] for c in ARG_ERRORS])
def test_argument_errors(lib, case, chain, over, words):
    """CNF_E_INVALID and a message naming the entry point, the argument and the stage, with nothing launched."""
    names = CHAINS[chain] if isinstance(chain, str) else chain
    with _Plans(lib, names) as plans:
        over = {k: (v(plans) if callable(v) else v) for k, v in over.items()}
        rc = _call(lib, plans, **over)
        msg = lib.cnf_last_error().decode()
        assert rc == -1 and msg, (case, rc, msg)
        assert 'cnf_flow_sample_cascade' in msg, (case, msg)
        for w in words:
            assert w in msg, (case, w, msg)
        if set(over) <= {'desc'} and case != 'null_desc':   # an error of the chain or the descriptor: no size either
            d = over.get('desc', _cdesc(L=len(plans)))
            assert lib.cnf_cascade_workspace_bytes(_arr([p.value for p in plans]), 2, C.byref(d)) == 0
            assert 'cnf_cascade_workspace_bytes' in lib.cnf_last_error().decode()


def test_valid_calls_get_as_far_as_sample(lib):
    """Valid arguments (one stage, two, three; all outputs, one output) are accepted, and then whatever
    cnf_flow_sample does with one stage's arguments: without a GPU both stop at the first HIP call with the same
    code. The addresses are placeholders, so with a GPU present nothing is called here."""
    if torch.cuda.is_available():
        return
    with _Plans(lib, CHAINS['one']) as plans:
        d = _desc()
        rc_ref = lib.cnf_flow_sample(plans[0], A, A, Y, C.byref(d), OUT, OUT + (1 << 30), OUT + (2 << 30), OUT + (3 << 30),
                                     WS, 2, None)
        msg_ref = lib.cnf_last_error().decode() if rc_ref else ''
        assert rc_ref != -1, msg_ref
        rc = _call(lib, plans, desc=_cdesc(L=1, S=(4,)))
        msg = lib.cnf_last_error().decode() if rc else ''
        assert rc == rc_ref, (rc, msg, rc_ref, msg_ref)
        assert msg.replace('cnf_flow_sample_cascade', 'cnf_flow_sample') == msg_ref
    for chain, S in (('x1', (3, 4)), ('x1L3', (2, 3, 2)), ('x3', (4, 1)), ('x2', (1, 5))):
        with _Plans(lib, CHAINS[chain]) as plans:
            L = len(plans)
            only_block_dev = dict(_NO_OUTPUT, block_dev=_arr([None] * (L - 1) + [OUT]))
            for over in ({}, _NO_SCORES, only_block_dev, dict(desc=_cdesc(L=L, S=S, residual=1, logit_a=0.01))):
                over = dict(dict(desc=_cdesc(L=L, S=S)), **over)
                assert _call(lib, plans, **over) == rc_ref, (chain, lib.cnf_last_error())


@pytest.mark.parametrize('chain', ['one', 'x1', 'x1L3', 'x3', 'x2'])
def test_cascade_workspace_bytes(lib, chain):
    """Exactly the sum over the stages of cnf_plan_sample_workspace_bytes (the plan's inverse workspace for `chunk`
    images + one chunk each of zy and xy_hat + the 3 B H_l W_l x_d state, whose terms test_sampling checks);
    independent of every S_l; growing with chunk and with B."""
    with _Plans(lib, CHAINS[chain]) as plans:
        L = len(plans)
        pa = _arr([p.value for p in plans])

        def size(B, S, chunk):
            d = _cdesc(L=L, S=S, chunk=chunk)
            return int(lib.cnf_cascade_workspace_bytes(pa, B, C.byref(d)))
        for B, chunk in [(1, 1), (2, 3), (2, 64), (8, 64), (5, 7)]:
            d1 = _desc(S=3, chunk=chunk)
            parts = [int(lib.cnf_plan_sample_workspace_bytes(p, B, C.byref(d1))) for p in plans]
            for kw, part in zip((_capi_kw(n) for n in CHAINS[chain]), parts):
                H, W, D = kw['io_shape']
                assert part >= 2 * chunk * H * W * D * 4 + 3 * B * H * W * kw['x_d'] * 4
            assert all(parts) and size(B, (3,) * L, chunk) == sum(parts), (B, chunk, parts)
            assert len({size(B, S, chunk) for S in [(1,) * L, (7,) * L, (1000, 2, 1, 1)[:L], (2, 1000, 50, 1)[:L]]}) == 1
        for chunk in (1, 3, 64):
            s = [size(B, (2,) * L, chunk) for B in range(1, 12)]
            assert s == sorted(s) and s[-1] > s[0]
        for B in (1, 4):
            s = [size(B, (2,) * L, chunk) for chunk in range(1, 70)]
            assert s == sorted(s) and s[-1] > s[0]


def test_cflowcascade_refuses_a_broken_chain():
    """cFlowCascade(flows) checks the chain once (io_d == 2 x_d, equal x_d, doubled height and width, one device,
    1..4 stages) and raises ValueError naming the stage. It reads io_shape, x_d and device alone, so stand-ins
    serve on the host."""
    from arl_conditional_normalizing_flows_amd.make_model import cFlowCascade

    def f(name, device='cuda:0'):
        return types.SimpleNamespace(io_shape=list(FLOWS[name]['io_shape']), x_d=FLOWS[name]['x_d'], device=device)
    for names in CHAINS.values():
        assert len(cFlowCascade([f(n) for n in names]).flows) == len(names)
    for flows, words in [([], ('stages',)), ([f('s4')] * 5, ('stages',)), ([f('small')], ('stage 1', 'io_d')),
                         ([f('s4'), f('v8')], ('stage 2', 'x_d')), ([f('s4'), f('s16')], ('stage 2', 'io_shape')),
                         ([f('s4'), f('s8'), f('s8')], ('stage 3', 'io_shape')),
                         ([f('s4'), f('s8', 'cuda:1')], ('stage 2', 'device'))]:
        with pytest.raises(ValueError) as e:
            cFlowCascade(flows)
        for w in words:
            assert w in str(e.value), (w, str(e.value))
    c = cFlowCascade([f(n) for n in CHAINS['x1L3']])
    # offset_l = offset + sum_{k<l} B N_k H_k W_k x_d
    assert c.default_offsets(2, (2, 3, 2), 5) == [5, 5 + 2 * 2 * 16, 5 + 2 * 2 * 16 + 2 * 6 * 64]


# ---------------------------------------------------------------------------------------------
# the block_dev bound, from the kernel's own operations
# ---------------------------------------------------------------------------------------------

def block_dev_bound(v, y):
    """(ref, bound) for block_dev of fp32 values v and conditions y [..., H, W, C], per leading index, u = 2^-24,
    w = 2^-53. k_block_dev per element (2x2 block, channel): t_k = (double)v_k - (double)y_k for the block's four
    pixels (one fp64 rounding each at the most: relative w), d = ((t_0 + t_1) + t_2) + t_3 (three fp64 additions),
    a = |0.25 d| (exact): |a - a_exact| <= gamma_4 * 0.25 sum_k |t_k| =: gamma_4 q. A lane adds its
    ceil(n / 64) elements in order and the butterfly adds 6 more levels: every a passes through at most
    ceil(n / 64) + 6 fp64 additions of non-negative numbers, so |s - sum a| <= gamma_{ceil(n/64)+6} sum a, and
    sum a <= Q = sum q. The float64 restatement below has the same terms and numpy's own summation order (at most
    n - 1 additions). Together, generously: (n + 16) 2w Q. The result rounds once to fp32: u (ref + that).
    ref = 0 exactly where every t_k is 0: the bound is then 0."""
    v, y = np.asarray(v), np.asarray(y)
    assert v.dtype == np.float32 and y.dtype == np.float32 and v.shape == y.shape
    t = v.astype(np.float64) - y.astype(np.float64)
    H, W, Cc = t.shape[-3:]
    t = t.reshape(t.shape[:-3] + (H // 2, 2, W // 2, 2, Cc))
    d = ((t[..., 0, :, 0, :] + t[..., 0, :, 1, :]) + t[..., 1, :, 0, :]) + t[..., 1, :, 1, :]
    ref = np.abs(0.25 * d).sum((-3, -2, -1))
    Q = (0.25 * np.abs(t)).sum((-5, -4, -3, -2, -1))
    n = (H // 2) * (W // 2) * Cc
    e64 = (n + 16) * 2.0 ** -52 * Q
    return ref, U * (ref + e64) + e64


def test_block_dev_bound_holds_for_the_rule_in_numpy():
    """The kernel's order restated in numpy (lane-strided fp64 sums, the xor butterfly, one fp32 rounding) against
    block_dev_bound on seeded values: the bound is a property of the rule, checked without a GPU."""
    rng = np.random.default_rng(0)
    for shape in [(5, 4, 4, 1), (3, 12, 20, 3), (2, 16, 16, 2)]:
        y = rng.standard_normal(shape).astype(np.float32)
        v = (y + 0.1 * rng.standard_normal(shape)).astype(np.float32)
        v[0] = y[0]
        ref, bound = block_dev_bound(v, y)
        assert ref[0] == 0 and bound[0] == 0
        H, W, Cc = shape[1:]
        t = v.astype(np.float64) - y.astype(np.float64)
        for i in range(shape[0]):
            a = []
            for bh in range(H // 2):
                for bx in range(W // 2):
                    for c in range(Cc):
                        d = 0.0
                        for k in range(4):
                            d += t[i, 2 * bh + (k >> 1), 2 * bx + (k & 1), c]
                        a.append(abs(0.25 * d))
            lanes = np.zeros(64)
            for e, val in enumerate(a):
                lanes[e % 64] += val
            for m in (32, 16, 8, 4, 2, 1):
                lanes = lanes + lanes[np.arange(64) ^ m]
            got = float(np.float32(lanes[0]))
            assert abs(got - ref[i]) <= bound[i], (shape, i, got, ref[i], bound[i])


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _flow(name, seed, zero_last_conv=False):
    from arl_conditional_normalizing_flows_amd.make_model import cFlow
    kw = FLOWS[name]
    flow = cFlow(**kw)
    ora = OracleCFlow(**kw)
    flow.set_weights(ora.init_params(seed, zero_last_conv=True) if zero_last_conv else ora.init_params(seed))
    return flow


@functools.lru_cache(maxsize=None)
def _cascade(chain, zero_last_conv=False):
    from arl_conditional_normalizing_flows_amd.make_model import cFlowCascade
    return cFlowCascade([_flow(n, l + 1, zero_last_conv) for l, n in enumerate(CHAINS[chain])])


def _y1(chain, B, seed=1):
    """`up` of a seeded uniform low-resolution batch: what preprocess_dataset_SR puts in the y channels"""
    from arl_conditional_normalizing_flows_amd.base_functions import up
    H, W, D = FLOWS[CHAINS[chain][0]]['io_shape']
    low = np.random.default_rng(seed).random((B, H // 2, W // 2, D // 2), dtype=np.float32)
    return up(torch.from_numpy(low).cuda()).contiguous()


# (id, chain, B, S, sampling keywords)
CASES = [
    ('x1-3x4', 'x1', 2, (3, 4), {}),
    ('x1-3x4-res', 'x1', 2, (3, 4), dict(residual=True)),
    ('x1-1x5-logit-res', 'x1', 3, (1, 5), dict(logit_a=0.01, residual=True)),
    ('x1L3-2x3x2', 'x1L3', 2, (2, 3, 2), {}),
    ('x1L3-2x3x2-res', 'x1L3', 3, (2, 3, 2), dict(residual=True)),
    ('x3-4x1-res', 'x3', 3, (4, 1), dict(residual=True)),
    ('x3-3x4', 'x3', 2, (3, 4), {}),
    ('x2-3x4-res', 'x2', 2, (3, 4), dict(residual=True)),
    ('one-5-logit-res', 'one', 2, (5,), dict(logit_a=0.01, residual=True)),
]
SEED, OFFSET = 7, 5
ALL = dict(return_stage_stats=True, return_y_dev=True, return_block_dev=True)


def _get(cid):
    return next(c for c in CASES if c[0] == cid)


@functools.lru_cache(maxsize=None)
def _composition(cid):
    """The chain by hand with the public calls of the parent commit: per stage the dict of cFlow.sample on the
    B N_{l-1} conditions (plus 'cond', those conditions), with the documented default offsets."""
    from arl_conditional_normalizing_flows_amd.base_functions import up
    _, chain, B, S, kw = _get(cid)
    cas = _cascade(chain)
    offs = cas.default_offsets(B, S, OFFSET)
    cond, stages = _y1(chain, B), []
    for f, s, o in zip(cas.flows, S, offs):
        out = f.sample(cond, s, seed=SEED, offset=o, return_y_dev=True, **kw)
        assert torch.isfinite(out['samples']).all()
        stages.append(dict(out, cond=cond))
        cond = up(out['samples'].reshape((-1,) + tuple(out['samples'].shape[2:]))).contiguous()
    return stages


@functools.lru_cache(maxsize=None)
def _case(cid):
    """(cascade, y1, B, S, kw, truth, hist box, the reference call's outputs at the default chunk)"""
    _, chain, B, S, kw = _get(cid)
    cas = _cascade(chain)
    leaves = _composition(cid)[-1]['samples']
    leaves = leaves.reshape((B, -1) + tuple(leaves.shape[2:]))
    truth = (leaves[:, min(2, leaves.shape[1] - 1)] + 0.05).contiguous()
    v = leaves.cpu().numpy().astype(np.float64)
    box = (BINS, float(np.floor(v.min() * 4) / 4 - 0.25), float(np.ceil(v.max() * 4) / 4 + 0.25))
    kw = dict(kw, seed=SEED, offset=OFFSET)
    ref = cas.sample(_y1(chain, B), S, truth=truth, hist=box, quantiles=LEVELS, **ALL, **kw)
    return cas, _y1(chain, B), B, S, kw, truth, box, ref


def _flat(out):
    """name -> tensor, the per-stage lists as name[l]"""
    flat = {}
    for n, t in out.items():
        if isinstance(t, list):
            flat.update({f'{n}[{l}]': x for l, x in enumerate(t)})
        else:
            flat[n] = t
    return flat


def _assert_same(got, ref, what):
    got, ref = _flat(got), _flat(ref)
    assert set(got) <= set(ref), (what, sorted(set(got) - set(ref)))
    for n, t in got.items():
        assert t.shape == ref[n].shape and same_bits(t, ref[n]), f'{what}: {n} differs'


@pytest.mark.gpu
@pytest.mark.parametrize('cid', [c[0] for c in CASES])
def test_cascade_equals_the_composition_of_the_public_calls(gpu, cid):
    """samples == the last stage's samples of f1.sample -> up -> f2.sample -> ..., bit for bit; stage 1's mean, std
    and y_dev are f1.sample's; every deeper stage's y_dev is that stage's sample(...)['y_dev'] reshaped; one stage:
    cFlow.sample in every output it has (the scores included)."""
    cas, y1, B, S, kw, truth, box, out = _case(cid)
    comp = _composition(cid)
    L = len(S)
    N = np.cumprod(S)
    for n in ('samples', 'mean', 'std', 'rank', 'abs_err', 'sq_err', 'hist', 'hist_centers', 'quantiles'):
        assert n in out, n
    HL, WL, _ = cas.flows[-1].io_shape
    assert tuple(out['samples'].shape) == (B, N[-1], HL, WL, cas.x_d)
    assert same_bits(out['samples'], comp[-1]['samples'].reshape(out['samples'].shape)), 'the leaves differ'
    for n in ('mean', 'std'):
        assert same_bits(out['stage_' + n][0], comp[0][n]), f'stage 1 {n}'
        assert same_bits(out[n], out['stage_' + n][-1]), n
    for l in range(L):
        assert tuple(out['y_dev'][l].shape) == (B, N[l]) == tuple(out['block_dev'][l].shape)
        assert same_bits(out['y_dev'][l], comp[l]['y_dev'].reshape(B, N[l])), f'stage {l + 1} y_dev'
    if L == 1:
        one = cas.flows[0].sample(y1, S[0], return_y_dev=True, truth=truth, hist=box, quantiles=LEVELS, **kw)
        for n, t in one.items():
            got = out[n][0] if n == 'y_dev' else out[n]
            assert same_bits(got, t), n


@pytest.mark.gpu
@pytest.mark.parametrize('cid', ['x1-3x4-res', 'x1-1x5-logit-res', 'x1L3-2x3x2-res', 'x3-3x4', 'x2-3x4-res'])
def test_no_output_depends_on_chunk(gpu, cid):
    """chunk in {1, 3, N_L - 1, N_L + 1, >= every node}: identical bits of every output, scores and per-stage lists
    included. With S_2 = 4 a chunk of 3 makes the child chunks 3, 3, 3, 3 of a parent chunk's 12 children: they
    straddle parents, and the parent chunks of 3 straddle the conditions."""
    cas, y1, B, S, kw, truth, box, ref = _case(cid)
    NL = int(np.prod(S))
    for chunk in (1, 3, max(NL - 1, 2), NL + 1, 4 * B * NL):
        got = cas.sample(y1, S, chunk=chunk, truth=truth, hist=box, quantiles=LEVELS, **ALL, **kw)
        assert sorted(got) == sorted(ref)
        _assert_same(got, ref, f'{cid} chunk={chunk}')


@pytest.mark.gpu
@pytest.mark.parametrize('cid', ['x1L3-2x3x2-res', 'x3-3x4'])
def test_outputs_ignore_prior_buffer_contents(gpu, cid):
    """The C ABI on output buffers and a workspace prefilled with the PATTERNS of test_state_independence (zeros,
    0xFF, another call's leftovers) between guard bands: the same bytes under every pattern, the guards
    untouched, and the bits of cFlowCascade.sample."""
    cas, y1, B, S, kw, truth, box, ref = _case(cid)
    lib = _lib.load()
    L, x_d = len(S), cas.x_d
    N = [int(n) for n in np.cumprod(S)]
    desc = _cdesc(L=L, S=S, chunk=4, seed=SEED, logit_a=kw.get('logit_a', 0.0), residual=int(kw.get('residual', False)))
    for l, o in enumerate(cas.default_offsets(B, S, OFFSET)):
        desc.offset[l] = o
    sd = _score_desc(box[0], box[1], box[2], LEVELS)
    plans = _arr([f._plan.value for f in cas.flows])
    nbytes = int(lib.cnf_cascade_workspace_bytes(plans, B, C.byref(desc)))
    assert nbytes > 0
    shp = [(B,) + tuple(f.io_shape[:2]) + (x_d,) for f in cas.flows]
    shapes = dict(ws=nbytes, samples=(B, N[-1]) + shp[-1][1:], rank=shp[-1], abs_err=shp[-1], sq_err=(B, N[-1]),
                  hist=shp[-1] + (box[0],), quantiles=(len(LEVELS),) + shp[-1])
    for l in range(L):
        shapes.update({f'stage_mean[{l}]': shp[l], f'stage_std[{l}]': shp[l], f'y_dev[{l}]': (B, N[l]),
                       f'block_dev[{l}]': (B, N[l])})
    names = [n for n in shapes if n != 'ws']
    y_other, truth_other = _y1(_get(cid)[1], B, seed=11), (truth * 0.5 - 0.3).contiguous()

    def call(b, y, t):
        raw = b.raw
        per = lambda n: _arr([raw[f'{n}[{l}]'].data_ptr() for l in range(L)])
        _lib.check(lib.cnf_flow_sample_cascade(
            plans, _arr([f.params.data_ptr() for f in cas.flows]), _arr([f._aux.data_ptr() for f in cas.flows]),
            y.data_ptr(), C.byref(desc), C.byref(sd), t.data_ptr(), raw['samples'].data_ptr(), raw['rank'].data_ptr(),
            raw['abs_err'].data_ptr(), raw['sq_err'].data_ptr(), raw['hist'].data_ptr(), raw['quantiles'].data_ptr(),
            per('stage_mean'), per('stage_std'), per('y_dev'), per('block_dev'), raw['ws'].data_ptr(), B,
            torch.cuda.current_stream().cuda_stream), 'cnf_flow_sample_cascade')
    res = {}
    for pat in PATTERNS:
        b = Buffers(pat, **shapes)
        if pat == 'L':
            call(b, y_other, truth_other)
        call(b, y1, truth)
        b.check(f'cascade {cid}')
        res[pat] = {n: b.raw[n].clone() for n in names}
    flat = _flat(ref)
    for pat in PATTERNS[1:]:
        for n in names:
            assert torch.equal(res[pat][n], res['Z'][n]), f'{n} under {pat} differs from Z'
    for n in names:
        assert torch.equal(res['Z'][n], flat[n].contiguous().view(-1).view(torch.uint8)), n


@pytest.mark.gpu
@pytest.mark.parametrize('cid', ['x1-3x4-res', 'x1L3-2x3x2', 'x2-3x4-res'])
def test_outputs_do_not_depend_on_the_other_outputs(gpu, cid):
    """Each group of outputs asked for alone, and the call without the samples: the bits of the full call, and
    exactly the keys asked for."""
    cas, y1, B, S, kw, truth, box, ref = _case(cid)
    none = dict(return_samples=False, return_stats=False)
    a = dict(chunk=4, **kw)
    runs = [
        ('no samples', dict(return_samples=False, truth=truth, hist=box, quantiles=LEVELS, **ALL),
         set(ref) - {'samples'}),
        ('samples only', dict(return_stats=False), {'samples'}),
        ('leaf stats only', dict(return_samples=False), {'mean', 'std'}),
        ('stage stats only', dict(none, return_stage_stats=True), {'stage_mean', 'stage_std'}),
        ('y_dev only', dict(none, return_y_dev=True), {'y_dev'}),
        ('block_dev only', dict(none, return_block_dev=True), {'block_dev'}),
        ('truth only', dict(none, truth=truth), {'rank', 'abs_err', 'sq_err'}),
        ('no sq_err', dict(none, truth=truth, return_sq_err=False), {'rank', 'abs_err'}),
        ('hist only', dict(none, hist=box), {'hist', 'hist_centers'}),
        ('quantiles', dict(none, hist=box, quantiles=LEVELS), {'hist', 'hist_centers', 'quantiles'}),
    ]
    for what, over, keys in runs:
        got = cas.sample(y1, S, **dict(a, **over))
        assert set(got) == keys, (what, sorted(got))
        _assert_same(got, ref, f'{cid} {what}')
    with pytest.raises(AssertionError):
        cas.sample(y1, S, **dict(a, **none))


@pytest.mark.gpu
@pytest.mark.parametrize('cid', [c[0] for c in CASES])
def test_stage_mean_and_std(gpu, cid):
    """Per stage, mean / std against the float64 statistics of that stage's samples (the leaves the call returns;
    the deeper stages' from the composition, which test 1 ties to the cascade) within test_sampling.stats_bounds: the
    fold is the same serial fold over N_l values in node order, so that bound applies unchanged."""
    cas, y1, B, S, kw, truth, box, out = _case(cid)
    comp = _composition(cid)
    for l in range(len(S)):
        s = out['samples'] if l == len(S) - 1 else comp[l]['samples']
        s = s.reshape((B, -1) + tuple(s.shape[2:])).cpu().numpy()
        mean, std, e_mean, e_std = stats_bounds(s)
        dm = np.abs(out['stage_mean'][l].cpu().numpy().astype(np.float64) - mean)
        ds = np.abs(out['stage_std'][l].cpu().numpy().astype(np.float64) - std)
        rm = np.max(np.where(dm > 0, dm / np.where(e_mean > 0, e_mean, 1e-300), 0.0))
        rs = np.max(np.where(ds > 0, ds / np.where(e_std > 0, e_std, 1e-300), 0.0))
        print(f'{cid} stage {l + 1} (N={s.shape[1]}): mean worst err/bound {rm:.3f}, std worst err/bound {rs:.3f}, '
              f'std <= {std.max():.3e}')
        assert np.all(dm <= e_mean), (cid, l, rm)
        assert np.all(ds <= e_std), (cid, l, rs)
        if s.shape[1] > 1:
            assert std.max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize('cid', [c[0] for c in CASES])
def test_leaf_scores(gpu, cid):
    """rank and hist integer-equal to numpy fp32 on the returned leaves; abs_err within abs_err_bound, sq_err within
    SQ_RTOL, the quantiles within quantile_bounds: test_sample_score's bounds with S = N_L."""
    cas, y1, B, S, kw, truth, box, out = _case(cid)
    NL = int(np.prod(S))
    rank, hist, inr = _np_rank_hist(out['samples'], truth, box)
    got_r, got_h = out['rank'].cpu().numpy(), out['hist'].cpu().numpy()
    assert out['rank'].dtype == torch.int32 and out['hist'].dtype == torch.int32
    assert np.array_equal(got_r, rank), f'{cid}: {np.count_nonzero(got_r != rank)} of {rank.size} ranks differ'
    assert np.array_equal(got_h, hist), f'{cid}: {np.count_nonzero(got_h != hist)} of {hist.size} counts differ'
    assert inr.all() and np.all(got_h.sum(-1) == NL)
    assert got_r.min() >= 1   # the truth sits just above one leaf
    s, t = out['samples'].cpu().numpy(), truth.cpu().numpy()
    m, bound = abs_err_bound(s, t)
    e = np.abs(out['abs_err'].cpu().numpy().astype(np.float64) - m)
    d = s.astype(np.float64) - t.astype(np.float64)[:, None]
    sq = (d * d).reshape(B, NL, -1).sum(-1)
    rel = np.abs(out['sq_err'].cpu().numpy().astype(np.float64) - sq) / sq
    want, tol, empty = quantile_bounds(s, box[1], box[2], box[0], LEVELS)
    eq = np.abs(out['quantiles'].cpu().numpy().astype(np.float64) - want)
    print(f'{cid}: N_L={NL} abs_err worst err/bound {np.max(e / np.where(bound > 0, bound, 1e-300)):.3f}; sq_err worst '
          f'rel err {rel.max():.3e} (bound {SQ_RTOL:.3e}); quantiles worst |diff| {eq.max():.4f} of {tol:.4f}')
    assert m.max() > 0 and sq.min() > 0 and not empty.any()
    assert np.all(e <= bound)
    assert np.all(rel <= SQ_RTOL)
    assert np.all(eq <= tol)


@pytest.mark.gpu
@pytest.mark.parametrize('cid', [c[0] for c in CASES])
def test_block_dev(gpu, cid):
    """Per stage against the float64 restatement on that stage's samples and conditions (the composition's, which
    test 1 ties to the cascade bit for bit) within block_dev_bound."""
    cas, y1, B, S, kw, truth, box, out = _case(cid)
    comp = _composition(cid)
    for l, st in enumerate(comp):
        v = st['samples'].cpu().numpy()                       # [conditions, S_l, H, W, C]
        y = np.broadcast_to(st['cond'].cpu().numpy()[:, None], v.shape)
        ref, bound = block_dev_bound(v, np.ascontiguousarray(y))
        got = out['block_dev'][l].cpu().numpy().astype(np.float64).reshape(ref.shape)
        e = np.abs(got - ref)
        print(f'{cid} stage {l + 1}: block_dev {ref.min():.3e} .. {ref.max():.3e}, worst err/bound '
              f'{np.max(np.where(e > 0, e / np.where(bound > 0, bound, 1e-300), 0.0)):.3f}')
        assert ref.max() > 0
        assert np.all(e <= bound), (cid, l)


@pytest.mark.gpu
@pytest.mark.parametrize('chain,S', [('x1', (3, 4)), ('x1L3', (2, 3, 2)), ('x3', (2, 3))])
def test_temperature_zero_gives_identical_leaves(gpu, chain, S):
    """temperature 0: every node of a stage has the latent 0 and, by induction, the condition of its siblings, so
    all leaves of a condition are identical and every stage's std is exactly 0."""
    cas, B = _cascade(chain), 2
    out = cas.sample(_y1(chain, B), S, temperature=0.0, seed=3, residual=True, chunk=5, return_stage_stats=True)
    leaves = out['samples']
    assert torch.isfinite(leaves).all()
    assert torch.equal(leaves, leaves[:, :1].expand_as(leaves))
    for l, sd in enumerate(out['stage_std']):
        assert torch.count_nonzero(sd) == 0, f'stage {l + 1}'
    assert torch.equal(out['mean'], leaves[:, 0])
    # per stage: only the last stage at temperature 0 still gives S_L identical children per parent
    T = (1.0,) * (len(S) - 1) + (0.0,)
    leaves = cas.sample(_y1(chain, B), S, temperature=T, seed=3, residual=True, return_stats=False)['samples']
    fam = leaves.reshape((B, -1, S[-1]) + tuple(leaves.shape[2:]))
    assert torch.equal(fam, fam[:, :, :1].expand_as(fam)) and not torch.equal(leaves, leaves[:, :1].expand_as(leaves))


@pytest.mark.gpu
@pytest.mark.parametrize('chain,S', [('x1', (3, 4)), ('x1L3', (2, 3, 2)), ('x2', (2, 3))])
def test_identity_flows_reproduce_the_upscaled_condition(gpu, chain, S):
    """Flows with the last conv of every s, t net zeroed are the identity; with residual=True and temperature 0
    every value is 0 + its condition, so every leaf equals up^(L-1)(y_1) exactly and every block_dev and y_dev is
    exactly 0. At temperature 1 the leaves differ from it and block_dev is positive."""
    from arl_conditional_normalizing_flows_amd.base_functions import up
    cas, B = _cascade(chain, True), 3
    y1 = _y1(chain, B)
    out = cas.sample(y1, S, temperature=0.0, residual=True, chunk=4, return_y_dev=True, return_block_dev=True)
    want = y1
    for _ in S[1:]:
        want = up(want)
    assert torch.equal(out['samples'], want[:, None].expand_as(out['samples']))
    for l in range(len(S)):
        assert torch.count_nonzero(out['y_dev'][l]) == 0 and torch.count_nonzero(out['block_dev'][l]) == 0, l
    assert torch.count_nonzero(out['std']) == 0 and torch.equal(out['mean'], want)
    hot = cas.sample(y1, S, temperature=1.0, residual=True, return_stats=False, return_block_dev=True)
    for l in range(len(S)):
        assert torch.all(hot['block_dev'][l] > 0), l
