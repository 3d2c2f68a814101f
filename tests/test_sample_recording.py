"""The recorded launches of the sampling calls (cnf_plan_num_recorded_launches / cnf_plan_recorded_launch_info):
per chunk the latent, the inverse's own launches (cnf_debug_schedule for the chunk's size) and the launches that
follow a chunk's inverse, in one fixed order, then one k_sample_quantiles. The sampler's names are literal lists
here, so the per-chunk output path of cnf_flow_sample and its kin and of cnf_flow_sample_cascade is pinned name by
name; the bits those launches compute are the other sampling suites'.

Single flow: preset 'tiny', B = 2, S = 3, chunk = 2: the chunks [0,1], [2,3], [4,5], the middle one straddling
the two conditions. Cascade: the chain 4x4x2 -> 8x8x2 (x_d 1), B = 2, S = (2, 3), chunk = 2: two chunks of stage 1,
each followed by the three chunks of its six children."""
import ctypes as C

import pytest

from arl_conditional_normalizing_flows_amd import _lib

from test_cascade_sampling import ALL, BINS, LEVELS, _cascade, _y1
from test_inverse_logdet import _schedule
from test_sampling import _flow, _y

BOX = (BINS, -4.0, 4.0)


def _launch_names(plan):
    lib = _lib.load()
    buf = C.create_string_buffer(256)
    names = []
    for i in range(lib.cnf_plan_num_recorded_launches(plan)):
        _lib.check(lib.cnf_plan_recorded_launch_info(plan, i, buf, 256, None, None), 'info')
        names.append(buf.value.decode())
    return names


def _is_sampler(name):
    return name.startswith(('k_latent', 'k_child_latent', 'k_sample_', 'k_block_dev'))


def _split(names):
    """(the sampler's launches in order, the other launches in the runs between them)"""
    own, runs = [], []
    for n in names:
        if _is_sampler(n):
            own.append(n)
            runs.append([])
        else:
            assert runs, names   # (a recording starts with a latent)
            runs[-1].append(n)
    return own, runs


def _assert_inverse_runs(own, runs, inverse, what):
    """after every latent the chunk's inverse, and nothing else anywhere"""
    for n, run in zip(own, runs):
        assert run == (inverse if n in ('k_latent', 'k_child_latent') else []), (what, n, run)


@pytest.mark.gpu
def test_single_flow_recording(gpu):
    flow, ora, P = _flow('tiny')
    lib = _lib.load()
    y = _y('tiny', 2)
    truth = y[..., :1].contiguous() * 0.5
    kw = dict(chunk=2, seed=3, offset=1, return_y_dev=True)

    flow.sample(y, 3, return_log_prob=True, truth=truth, hist=BOX, quantiles=LEVELS, **kw)
    own, runs = _split(_launch_names(flow._plan))
    chunk = ['k_latent', 'k_sample_fold', 'k_sample_ydev', 'k_sample_logp', 'k_sample_score', 'k_sample_sqerr']
    assert own == chunk * 3 + ['k_sample_quantiles']
    scored = (own, runs)

    flow.sample(y, 3, **kw)
    own, runs = _split(_launch_names(flow._plan))
    assert own == ['k_latent', 'k_sample_fold', 'k_sample_ydev'] * 3
    inv = _schedule(lib, flow._plan, 2, -1)
    _assert_inverse_runs(own, runs, inv, 'cnf_flow_sample')
    # with log_prob the inverse leaves its log-det slots to k_sample_logp: the -2 schedule less its reduce
    slots = [n for n in _schedule(lib, flow._plan, 2, -2) if n != 'k_ld_reduce']
    _assert_inverse_runs(*scored, slots, 'cnf_flow_sample_score')


@pytest.mark.gpu
def test_cascade_recording(gpu):
    cas = _cascade('x1')
    lib = _lib.load()
    B, S = 2, (2, 3)
    y1 = _y1('x1', B)
    H, W, _ = cas.flows[-1].io_shape
    truth = y1.new_full((B, H, W, cas.x_d), 0.25)
    cas.sample(y1, S, chunk=2, seed=3, offset=1, truth=truth, hist=BOX, quantiles=LEVELS, return_sq_err=True, **ALL)
    node = ['k_sample_fold_node', 'k_sample_ydev_node', 'k_block_dev']
    want = [
        # stage 1: B S_1 = 4 nodes in 2 chunks
        (['k_latent'] + node) * 2,
        # stage 2: the 6 children of each stage-1 chunk in 3 chunks, after that chunk: 6 chunks in all; the leaf
        # plan alone scores, and ends with the quantiles
        (['k_child_latent'] + node + ['k_sample_score_node', 'k_sample_sqerr_node']) * 6 + ['k_sample_quantiles'],
    ]
    recorded = [_split(_launch_names(f._plan)) for f in cas.flows]
    for l, f in enumerate(cas.flows):
        own, runs = recorded[l]
        assert own == want[l], (l, own)
        _assert_inverse_runs(own, runs, _schedule(lib, f._plan, 2, -1), f'stage {l + 1}')
