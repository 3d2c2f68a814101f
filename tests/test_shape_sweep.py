"""The flow kernels at shapes config.PRESETS never reaches.

Every other GPU test builds its flow from a preset: square images, even depth, num_kernels in
{8, 16, 32, 64}, DILATIONS=True, 1 to 3 residual blocks. The host code picks kernels, packings and
fallbacks from predicates on exactly these quantities (dc1 % 4, nk % 4, 9*cout <= nk, gc % 4, W % 4,
W >= 4, the 64-pixel k_pw tile count, the k_gc tile picker), so with the presets each takes one side on
every run. SWEEP holds, per edge, the smallest flow that reaches it (it is not part of PRESETS: the
golden generator and the shape-table generator enumerate that).

CPU part (against the cross-compiled library, no GPU): the plan of every row agrees with the oracle;
a plan that cnf_plan_create accepts can be scheduled in both directions (what the schedules cannot
run is refused at creation); the launch names the sweep claims to cover are in its dry runs.

GPU part: forward, per-image log-det, inverse, NLL and the training gradient against the float64
oracles under the bounds of test_gpu_parity.py / test_train.py (imported, not restated), and the
bit-for-bit properties (layerwise == fused, batch independence) on the same rows.

Inputs are standard normal (np.random.default_rng(seed)), weights OracleCFlow.init_params(seed)."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

from arl_conditional_normalizing_flows_amd import _lib
from arl_conditional_normalizing_flows_amd.config import PRESETS
from oracle.cflow_np import OracleCFlow

from test_capi import _plan, check_plan_matches_oracle, schedule_of_plan
from test_gpu_parity import KNOBS, RTOL, _err, check_logdet


def _row(io_shape, x_d, squeeze, resnext, nk, card, **extra):
    return dict(io_shape=list(io_shape), x_d=x_d, squeeze_factor_block_list=list(squeeze),
                ResNeXt_block_list=list(resnext), num_kernels_list=list(nk), cardinality_list=list(card), **extra)


_SMALL = ((0, 1, 0), (2, 1, 1), (16, 16, 8), (4, 4, 2))
_RECT = ((0, 1, 0), (1, 1, 1), (16, 16, 8), (4, 4, 2))
# ordered from the most preset-like row to the least (the order the GPU cases run in)
SWEEP = {
    # one-branch grouped stage everywhere
    'nodil': _row((16, 16, 4), 3, *_SMALL, DILATIONS=False),
    # forward / inverse without LayerNorm (the presets run it in the training tests only)
    'noln': _row((16, 16, 4), 3, *_SMALL, LAYER_NORM=False),
    # W = 3H: compressed layers 4x12 and 2x6
    'wide': _row((8, 24, 4), 3, *_RECT),
    # H = 3W: the transpose of 'wide' (a swapped H / W)
    'tall': _row((24, 8, 4), 3, *_RECT),
    # streamed by default on a non-square image: k_gc tiles, dilations 1, 2, 4, 1536 pixels = 24 k_pw tiles;
    # the second block mixes LDS and streamed layers
    'rect32x48': _row((32, 48, 4), 3, (0, 1), (1, 1), (64, 32), (8, 4)),
    # nk 24 / 12: branch widths 6 and 3, gc = 36 / 18
    'nk24': _row((16, 16, 4), 3, (0, 1), (1, 1), (24, 24), (2, 2)),
    # k_pw nr = 3; layers 2, 3 of each block are streamed by default
    'nk48': _row((16, 16, 4), 3, (0, 0), (1, 1), (48, 48), (4, 4)),
    # a block with no residual blocks
    'r0': _row((8, 8, 4), 3, (0, 1), (0, 1), (8, 8), (2, 2)),
    # R = 4, D = 2: dc = 1 on the channel masks
    'r4': _row((8, 8, 2), 1, (0,), (4,), (16,), (2,)),
    # x_d = 1 of 4: NLL and factor split off the presets' x_d = D - 1
    'xd1of4': _row((8, 8, 4), 1, (0, 1), (1, 1), (8, 8), (2, 2)),
    # odd D: channel masks with (dc1, dc2) = (2, 1), (1, 2); k_pw<1,1,conv_in/out> when streamed
    'odd_d3': _row((16, 16, 3), 2, *_SMALL),
    # odd D with (3, 2), (2, 3); checkerboard dc1 = 10, not a multiple of 4
    'odd_d5': _row((8, 8, 5), 3, (0, 1), (1, 1), (8, 8), (2, 2)),
    # widths 6, 10, 5, 3: the W % 4 != 0 and W < 4 weight-gradient fallbacks; 15- and 60-pixel images
    # (partial 16-pixel wave tiles)
    'w12x20': _row((12, 20, 4), 3, (1, 0), (1, 1), (16, 8), (4, 2)),
    # compressed images down to 1x1 and 2x2
    'min4x4': _row((4, 4, 2), 1, (1, 0), (1, 1), (8, 8), (2, 2)),
    # checkerboard layers 8x1 (compressed width 1)
    'w2': _row((16, 2, 4), 3, (0,), (1,), (8,), (2,)),
}
ROWS = list(SWEEP)

# the configuration the kernels cannot run: 128-channel convolutions in streamed layers
NK128 = _row((8, 8, 4), 3, (0,), (1,), (128,), (8,))
LIMIT_MSG = 'more than 64 output channels'


def _kw(name):
    """constructor arguments of cFlow / OracleCFlow / TorchCPUFlow for a sweep row"""
    return dict(SWEEP[name], group_mode='reference')


def _opt_str(opts):
    return ','.join(f'{k}={v}' for k, v in opts.items()) if opts else None


def _names(lib, kw, options=None, batches=(1, 3)):
    """the plan is created and both schedules dry-run at every batch; returns the set of launch names"""
    rc, p, keep = _plan(lib, kw, options=_opt_str(options))
    assert rc == 0, lib.cnf_last_error()
    try:
        out = set()
        for B in batches:
            for direction in (1, -1):
                out.update(schedule_of_plan(lib, p, B, direction))
        assert lib.cnf_plan_workspace_bytes(p, 3) > 0
        assert lib.cnf_plan_train_workspace_bytes(p, 3) > 0
        return out
    finally:
        lib.cnf_plan_destroy(p)


# ---------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ROWS)
def test_plan_matches_oracle(lib, name):
    check_plan_matches_oracle(lib, dict(SWEEP[name]))


@pytest.mark.parametrize('options', [None, {'NETLDS': 0}], ids=['default', 'streamed'])
@pytest.mark.parametrize('name', ROWS)
def test_sweep_plan_can_be_scheduled(lib, name, options):
    assert _names(lib, SWEEP[name], options)


def _wider_list():
    """shapes around the sweep's: every combination is either refused by cnf_plan_create or schedulable"""
    out = []
    for (H, W), D, nk, card, sq in itertools.product([(4, 4), (12, 20), (16, 16), (32, 48)], (3, 8),
                                                      (8, 24, 64, 96, 128), (2, 8), ((0,), (1, 0))):
        n = len(sq)
        for dil in (True, False):
            out.append(_row((H, W, D), D - 1, sq, (1,) * n, (nk,) * n, (card,) * n, DILATIONS=dil))
    return out


def test_a_created_plan_can_be_scheduled(lib):
    """Whenever cnf_plan_create returns 0 with default options, cnf_debug_schedule succeeds in both
    directions at B = 1 and B = 3 (and at a batch the image-looping launches size differently, 70);
    whenever it does not, there is a message. Over the presets, the sweep and a wider list around it."""
    created = refused = 0
    cases = [(dict(PRESETS[n].kwargs()), gm) for n in PRESETS for gm in (0, 1)]   # both group modes
    cases += [(kw, 0) for kw in [SWEEP[n] for n in ROWS] + [NK128] + _wider_list()]
    for kw, gm in cases:
        kw = {k: v for k, v in kw.items() if k != 'group_mode'}
        # (a CNF_GROUP_INTENDED plan is dry-run at creation only when asked: include/cnf.h)
        rc, p, keep = _plan(lib, kw, gm, 'SCHEDULE_CHECK=1' if gm else None)
        if rc != 0:
            refused += 1
            assert not p.value and lib.cnf_last_error(), kw
            continue
        created += 1
        try:
            for B in (1, 3, 70):
                for direction in (1, -1):
                    assert schedule_of_plan(lib, p, B, direction), kw
        finally:
            lib.cnf_plan_destroy(p)
    print(f'{created} plans created and scheduled, {refused} refused')
    assert created >= 50 and refused >= 50


# what plan creation says to the presets with every layer streamed (NETLDS=0): all of them can run. The
# streamed kernels take at most 64 output channels per problem, and the one convolution of the presets
# that is wider, conv_out of cfg4's / cfg5's deepest blocks (dc2 = 96 .. 192), is split into 64-channel
# chunks (cnf_plan.cpp co_chunks). A preset that turns False here must be refused with the limit's message.
PRESETS_STREAMED = {'tiny': True, 'small': True, 'narrow': True, 'cfg2': True, 'cfg3': True, 'ref_default': True,
                    'cfg4': True, 'cfg5': True}


@pytest.mark.parametrize('name', list(PRESETS))
def test_presets_streamed_plan_or_refuse(lib, name):
    kw = PRESETS[name].kwargs()
    kw.pop('group_mode')
    rc, p, keep = _plan(lib, kw, options='NETLDS=0')
    if rc == 0:
        try:
            for B in (1, 3):
                for direction in (1, -1):
                    assert schedule_of_plan(lib, p, B, direction)
        finally:
            lib.cnf_plan_destroy(p)
    else:
        assert rc == -1 and not p.value
        assert LIMIT_MSG in lib.cnf_last_error().decode()
    assert (rc == 0) == PRESETS_STREAMED[name]


def test_sweep_reaches_the_launches_it_claims(lib):
    """A planner change that silently drops these instantiations from the sweep is seen here."""
    seen = set()
    for name in ROWS:
        seen |= _names(lib, SWEEP[name]) | _names(lib, SWEEP[name], {'NETLDS': 0})
    for k in ('k_pw<3,2,conv_in>', 'k_pw<3,4,conv_a>', 'k_pw<3,8,conv_b>', 'k_pw<1,1,conv_in>', 'k_pw<1,1,conv_out>',
              'k_net_lds', 'k_gc'):
        assert any(s == k or s.startswith(k + '<') for s in seen), (k, sorted(seen))
    # the fallback kernels' scalar / unaligned variants
    for name in ('odd_d3', 'nk24', 'w12x20'):
        for knob in ('nogc', 'conv1'):
            seen |= _names(lib, SWEEP[name], KNOBS[knob])
    assert any(s.startswith('k_conv1<') for s in seen) and any(s.startswith('k_convtap<') for s in seen), sorted(seen)


def test_nk128_is_rejected_at_plan_creation(lib):
    rc, p, keep = _plan(lib, NK128)
    assert rc == -1 and not p.value
    assert LIMIT_MSG in lib.cnf_last_error().decode()
    from arl_conditional_normalizing_flows_amd.make_model import cFlow
    with pytest.raises(AssertionError, match=LIMIT_MSG):
        cFlow(**NK128, device='cpu')   # raises before anything is allocated
    # the reference's own asserts still come first
    rc, p, keep = _plan(lib, dict(NK128, cardinality_list=[3]))
    assert rc == -1 and 'cardinality' in lib.cnf_last_error().decode()


def test_intended_mode_is_refused_where_it_cannot_run(lib):
    """The other configuration found to plan without being schedulable: group_mode 'intended' on a flow
    with streamed layers, whose dense grouped image exceeds LDS. cFlow refuses it at
    construction, as does cnf_plan_create when asked for the check (SCHEDULE_CHECK=1); through the C ABI
    an 'intended' plan is by default the tables alone (the host-side table tests of test_capi.py read
    them). The presets it runs on (tiny, small, narrow) plan either way."""
    from arl_conditional_normalizing_flows_amd.make_model import cFlow
    for name in PRESETS:
        kw = PRESETS[name].kwargs()
        kw.pop('group_mode')
        rc, p, keep = _plan(lib, kw, 1, 'SCHEDULE_CHECK=1')
        if name in ('tiny', 'small', 'narrow'):
            assert rc == 0, name
        else:
            assert rc == -1 and not p.value, name
            assert 'LDS budget' in lib.cnf_last_error().decode()
            with pytest.raises(AssertionError, match='LDS budget'):
                cFlow(**kw, group_mode='intended', device='cpu')   # raises before anything is allocated
            rc, p, keep = _plan(lib, kw, 1)
            assert rc == 0, name
        lib.cnf_plan_destroy(p)
    # the reference mode has no such default: SCHEDULE_CHECK=0 is the only way to an unrunnable plan
    rc, p, keep = _plan(lib, NK128, 0, 'SCHEDULE_CHECK=0')
    assert rc == 0
    lib.cnf_plan_destroy(p)


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _oracle(name, B=3, seed=0, lambda_y=100.0):
    """float64 numpy oracle of a row, computed once: weights, inputs, forward, inverse of its own zy"""
    kw = dict(_kw(name), lambda_y=lambda_y)
    ora = OracleCFlow(**kw)
    P = ora.init_params(seed)
    H, W, D = kw['io_shape']
    xy = np.random.default_rng(seed).standard_normal((B, H, W, D)).astype(np.float32)
    zy_ref, ld_ref, abs_s = ora.forward(xy, P, abs_s=True)
    x_ref = ora.inverse(zy_ref, P)
    for a in (xy, zy_ref, ld_ref, abs_s, x_ref):
        a.setflags(write=False)
    return kw, ora, P, xy, zy_ref, ld_ref, abs_s, x_ref


def _flow(kw, P, gpu, options=None):
    from arl_conditional_normalizing_flows_amd.make_model import cFlow
    flow = cFlow(**kw, device=gpu, debug_options=options)
    flow.set_weights(P)
    return flow


PARITY = ([(n, o) for n in ROWS for o in ('default', 'streamed')] +
          [(n, o) for n in ('odd_d3', 'nk24', 'w12x20') for o in ('nogc', 'conv1')])
_OPTS = dict(KNOBS, default=None, streamed={'NETLDS': 0})


@pytest.mark.gpu
@pytest.mark.parametrize('name,path', PARITY)
def test_forward_logdet_inverse_match_oracle(gpu, name, path):
    kw, ora, P, xy, zy_ref, ld_ref, abs_s, x_ref = _oracle(name)
    flow = _flow(kw, P, gpu, _OPTS[path])
    zy, ld = flow(torch.from_numpy(xy).to(gpu), 1, per_image_logdet=True)
    # the GPU inverse of the oracle's zy against the oracle's inverse
    x = flow(torch.from_numpy(zy_ref.astype(np.float32)).to(gpu), -1)
    torch.cuda.synchronize()
    e_zy = _err(zy.cpu().numpy(), zy_ref)
    e_x = _err(x.cpu().numpy(), x_ref)
    print(f'{name} {path}: zy rel err {e_zy:.3e} inverse rel err {e_x:.3e} (err/tol {e_zy / RTOL:.3f} {e_x / RTOL:.3f})')
    assert torch.isfinite(zy).all() and torch.isfinite(x).all()
    assert e_zy < RTOL
    assert e_x < RTOL
    check_logdet(ld.cpu().numpy(), ld_ref, abs_s, f'{name} {path}')


@pytest.mark.gpu
@pytest.mark.parametrize('name,lambda_y', [('xd1of4', 100.0), ('odd_d5', 100.0), ('xd1of4', 7.5)])
def test_nll_matches_oracle(gpu, name, lambda_y):
    kw, ora, P, xy, zy_ref, ld_ref, abs_s, x_ref = _oracle(name, lambda_y=lambda_y)
    ref = ora.log_loss(xy, P)
    got = [t.item() for t in _flow(kw, P, gpu).log_loss(torch.from_numpy(xy).to(gpu))]
    print(f'{name} lambda_y={lambda_y} nll', ref, got)
    for r, g in zip(ref, got):   # the bound of test_gpu_parity.test_nll_matches_oracle
        assert abs(r - g) <= RTOL * max(abs(r), abs_s.mean())


@pytest.mark.gpu
@pytest.mark.parametrize('name', ROWS)
def test_layerwise_equals_fused(gpu, name):
    """test_gpu_parity.test_layerwise_equals_fused on the sweep rows."""
    kw, ora, P, xy = _oracle(name)[:4]
    flow = _flow(kw, P, gpu)
    x = torch.from_numpy(xy).to(gpu)
    zy1, ld1 = flow(x, 1, per_image_logdet=True)
    zy2, ld2 = flow(x, 1, per_image_logdet=True, layerwise=True)
    xi1 = flow(zy1, -1)
    xi2 = flow(zy1, -1, layerwise=True)
    torch.cuda.synchronize()
    assert torch.equal(zy1, zy2)
    assert torch.allclose(ld1, ld2, rtol=1e-6, atol=1e-5)
    assert torch.equal(xi1, xi2)


@pytest.mark.gpu
@pytest.mark.parametrize('path', ['default', 'streamed'])
@pytest.mark.parametrize('name', ['nk48', 'rect32x48', 'odd_d3', 'w12x20'])
def test_batch_independence(gpu, name, path):
    """One batch of 7 against the same images in batches of 3 (the last one ragged): zy, per-image log-det
    and inverse equal bit for bit (test_gpu_parity.test_ragged_large_batch_matches_small_batches)."""
    kw, ora, P = _oracle(name)[:3]
    flow = _flow(kw, P, gpu, _OPTS[path])
    H, W, D = kw['io_shape']
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((7, H, W, D)).astype(np.float32)).to(gpu)
    zy, ld = flow(x, 1, per_image_logdet=True)
    xi = flow(zy, -1)
    assert torch.isfinite(zy).all() and torch.isfinite(ld).all() and torch.isfinite(xi).all()
    for s in range(0, 7, 3):
        zs, ls = flow(x[s:s + 3], 1, per_image_logdet=True)
        xs = flow(zy[s:s + 3], -1)
        assert torch.equal(zs, zy[s:s + 3]), (s, (zs - zy[s:s + 3]).abs().max().item())
        assert torch.equal(ls, ld[s:s + 3]), (s, (ls - ld[s:s + 3]).abs().max().item())
        assert torch.equal(xs, xi[s:s + 3]), (s, (xs - xi[s:s + 3]).abs().max().item())


GRAD_ROWS = ['nodil', 'wide', 'tall', 'nk24', 'nk48', 'r0', 'odd_d3', 'odd_d5', 'w12x20', 'min4x4', 'w2']
# the multi-kernel backward for the LDS layers too, on the odd shapes
GRAD_CASES = [(n, None) for n in GRAD_ROWS] + [(n, {'LDS_BWD': 0}) for n in ('odd_d3', 'w12x20')]


@functools.lru_cache(maxsize=None)
def _grad_refs(name):
    """float64 and fp32 autograd of a row at B = 2, computed once (shared by the LDS_BWD variants)"""
    from test_train import oracle_grads
    kw = _kw(name)
    H, W, D = kw['io_shape']
    xy = np.random.default_rng(6).standard_normal((2, H, W, D)).astype(np.float32)
    P = OracleCFlow(**kw).init_params(5)   # check_gradients' weights
    G_ref, terms_ref = oracle_grads(kw, P, xy)
    G32, _ = oracle_grads(kw, P, xy, torch.float32)
    return kw, xy, (G_ref, terms_ref, G32)


@pytest.mark.gpu
@pytest.mark.parametrize('name,options', GRAD_CASES)
def test_gradients_match_oracle(gpu, name, options):
    """test_train's bar per parameter tensor (K32, GRAD_RTOL, GRAD_ATOL; no perturbation term, as for
    the small presets) and its loss-term bound."""
    from test_train import check_gradients
    kw, xy, refs = _grad_refs(name)
    check_gradients(gpu, kw, xy, options, f'{name} {options or ""}', None, refs)
