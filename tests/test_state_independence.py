"""State independence: the outputs of a call are a function of its inputs and the weights only.

Every other GPU test hands a kernel the cached `torch.empty` workspace of its batch size and reuses it
for the same images, so a read of a workspace byte that nothing wrote in this call (an LN partial slot,
a pad column, a tail image, a gradient buffer that was never zeroed) sees the same batch's own data
and goes unnoticed, and so does a write outside a region. Here each entry point runs once per fill
pattern on a workspace and on output buffers that sit between guard bands:

  Z  every byte 0x00
  N  every byte 0xFF (every fp32 word a NaN, every int word -1)
  L  leftovers: the same entry point has just run on another batch of the same size

and the results must be equal BIT FOR BIT, finite, with every guard byte unchanged. The guard bands
hold the complement of the fill (0xFF around Z and L, 0x00 around N), so a read outside a buffer
changes a result as well. An oracle anchor (float64, the project's own bounds) keeps the three runs
from agreeing on one wrong answer; the last test compares a captured graph's replay with the eager
call. All checks are deterministic: one run per condition."""
import ctypes as C

import numpy as np
import pytest
import torch

from arl_conditional_normalizing_flows_amd import _lib
from arl_conditional_normalizing_flows_amd.config import PRESETS
from oracle.cflow_np import synthetic_class_batch, synthetic_sr_batch
from test_gpu_parity import KNOBS, RTOL, _err, _setup, check_logdet, ld_tol, torch64_forward  # noqa: F401

pytestmark = pytest.mark.gpu

G = 1 << 20   # guard band bytes on either side of a payload: a multiple of 4096, so the payload keeps the allocator's alignment
PATTERNS = ('Z', 'N', 'L')
FILL = {'Z': 0x00, 'N': 0xFF, 'L': 0x00}   # (L: the bytes the priming run leaves untouched are zeros)


def guarded(nbytes, fill):
    """(payload, check): a uint8 payload view of nbytes filled with `fill` inside one slab of G + nbytes + G
    bytes whose guard bands hold the complement of `fill`; check() synchronises and asserts that no guard
    byte changed."""
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
            assert bad.numel() == 0, (f'{what}: {bad.numel()} guard bytes {side} the buffer changed, the first '
                                      f'{int(bad[0]) - G if side == "below" else int(bad[0])} bytes {side} its '
                                      f'{"start" if side == "below" else "end"}')
    return payload, check


class Buffers:
    """Guarded device buffers of one fill pattern: raw[name] the uint8 payload, name -> its fp32 view."""

    def __init__(self, pat, **shapes):
        self.pat = pat
        self.raw, self.checks = {}, {}
        for name, shape in shapes.items():
            nbytes = int(shape) if name == 'ws' else 4 * int(np.prod(shape))
            self.raw[name], self.checks[name] = guarded(nbytes, FILL[pat])
            setattr(self, name, self.raw[name] if name == 'ws' else self.raw[name].view(torch.float32).reshape(shape))

    def refill(self, *names):
        for n in names:
            self.raw[n].fill_(FILL[self.pat])

    def check(self, what):
        for n, c in self.checks.items():
            c(f'{what} [{self.pat}] {n}')


def run_pattern(bufs, outputs, entry, args, other_args):
    """One run of `entry` under bufs.pat: Z / N refill the workspace and the outputs first, L runs the entry
    point on another batch and leaves every buffer as it is. Returns clones of the outputs."""
    if bufs.pat == 'L':
        entry(*other_args)
    else:
        bufs.refill('ws', *outputs)
    entry(*args)
    return [getattr(bufs, n).clone() for n in outputs]


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def max_diff(a, b):
    return float(torch.nan_to_num((a.double() - b.double()).abs(), nan=float('inf')).max())


def assert_patterns_agree(res, names, what):
    """res[pattern] = list of tensors (in the order of names): all finite and bit-equal to the Z run's."""
    for pat, outs in res.items():
        for n, t in zip(names, outs):
            assert torch.isfinite(t).all(), f'{what}: {n} under {pat} is not finite'
    for pat in PATTERNS[1:]:
        for n, a, b in zip(names, res['Z'], res[pat]):
            assert same_bits(a, b), f'{what}: {n} under {pat} differs from Z, max abs diff {max_diff(a, b):.3e}'


def _batch(name, B, seed):
    cfg = PRESETS[name]
    H, W, _D = cfg.io_shape
    xy = (synthetic_class_batch(B, H, W, cfg.x_d, seed=seed) if cfg.data == 'class'
          else synthetic_sr_batch(B, H, W, cfg.x_d, cfg.sr_pow, seed=seed))
    return torch.from_numpy(xy).cuda()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ws_bytes(flow, B):
    return int(_lib.load().cnf_plan_workspace_bytes(flow._plan, B))


def c_forward(flow, b, x):
    B = x.shape[0]
    _lib.check(_lib.load().cnf_flow_forward(flow._plan, flow.params.data_ptr(), flow._aux.data_ptr(), x.data_ptr(),
                                            b.zy.data_ptr(), b.ld.data_ptr(), flow._workspace(B).data_ptr(), B, _st()),
               'cnf_flow_forward')


def c_inverse(flow, b, z):
    B = z.shape[0]
    _lib.check(_lib.load().cnf_flow_inverse(flow._plan, flow.params.data_ptr(), flow._aux.data_ptr(), z.data_ptr(),
                                            b.xy.data_ptr(), flow._workspace(B).data_ptr(), B, _st()), 'cnf_flow_inverse')


def c_noise(flow, b, x, noise):
    B = x.shape[0]
    alpha, seed, offset, logit_a = (tuple(noise) + (0.0,))[:4]
    _lib.check(_lib.load().cnf_flow_forward_noise(flow._plan, flow.params.data_ptr(), flow._aux.data_ptr(), x.data_ptr(),
                                                  float(logit_a), float(alpha), int(seed), int(offset), b.xn.data_ptr(),
                                                  b.zy.data_ptr(), b.ld.data_ptr(), flow._workspace(B).data_ptr(), B,
                                                  _st()), 'cnf_flow_forward_noise')


# ---------------------------------------------------------------------------------------------
# 1. forward / inverse / log-det
# ---------------------------------------------------------------------------------------------

# (preset, B, netlds of _setup (True / False / a KNOBS key), further debug options, oracle anchor): the
# smallest batches at which each kernel family's image loop, tails and slot tables are live
FI_CASES = [
    ('small', 3, True, None, True), ('narrow', 3, True, None, True),     # LDS path; couplings 1 and 2 pixels wide
    ('small', 3, False, None, False),                                    # streamed
    ('cfg2', 5, 'nogc', None, True), ('cfg2', 5, 'conv1', None, True),   # fallback kernels
    ('cfg2', 17, True, None, False),    # smallest batch whose k_pw workgroups loop over 2 images (16 tiles * 2 nets * 17 > 512)
    ('cfg2', 64, True, None, False),    # the benched size: 4 images per k_pw workgroup
    ('cfg2', 67, True, None, False),    # the last workgroup has a partial image set
    ('cfg2', 17, False, None, False),   # every layer streamed
    ('cfg3', 67, True, None, False),    # 6-channel input
    ('cfg4', 6, True, None, False), ('cfg5', 2, True, None, False),   # 64x64 / 128x128, 2 images per workgroup, shipped default
    ('cfg4', 6, True, {'GENERIC': 0}, False), ('cfg5', 2, True, {'GENERIC': 0}, False),   # the specialised instantiations
    ('cfg4', 2, True, None, True),      # 64x64 against the oracle
]
FI_IDS = ['-'.join([c[0], f'B{c[1]}'] + ([] if c[2] is True else ['streamed' if c[2] is False else c[2]])
                   + [f'{k}{v}' for k, v in (c[3] or {}).items()]) for c in FI_CASES]

_oracle = {}


def oracle_forward(name, xy, P):
    """float64 (zy, per-image log-det, per-image sum|s|) of _setup's batch, computed once per (preset, B)."""
    key = (name, xy.shape[0])
    if key not in _oracle:
        _oracle[key] = torch64_forward(name, xy, P)
    return _oracle[key]


@pytest.mark.parametrize('direction', ['forward', 'inverse'])
@pytest.mark.parametrize('name,B,netlds,options,anchor', FI_CASES, ids=FI_IDS)
def test_flow_ignores_workspace_contents(gpu, name, B, netlds, options, anchor, direction):
    """cnf_flow_forward (zy, per-image log-det) / cnf_flow_inverse through the C ABI under Z, N and L: bit-equal,
    finite, no byte outside zy / logdet / xy / the workspace touched; the N run within the project's bounds of
    the float64 oracle where anchored."""
    flow, ora, P, xy = _setup(name, B, netlds=netlds, options=options)
    what = f'{name} B={B} {netlds} {options} {direction}'
    x, x_other = torch.from_numpy(xy).to(gpu), _batch(name, B, 11)
    if anchor:
        zy_ref, ld_ref, abs_s = oracle_forward(name, xy, P)
    if direction == 'forward':
        entry, outputs, inp, inp_other = c_forward, ('zy', 'ld'), x, x_other
    else:
        # the inverse of a fixed zy: the oracle's (its preimage is xy: the float64 flow inverts to 1e-12), else the flow's own
        inp = torch.from_numpy(zy_ref.astype(np.float32)).to(gpu) if anchor else flow(x, 1)[0]
        entry, outputs, inp_other = c_inverse, ('xy',), flow(x_other, 1)[0]
    res = {}
    for pat in PATTERNS:
        b = Buffers(pat, ws=_ws_bytes(flow, B), zy=x.shape, ld=(B,), xy=x.shape)
        flow._ws[B] = b.ws
        res[pat] = run_pattern(b, outputs, entry, (flow, b, inp), (flow, b, inp_other))
        b.check(what)
    assert_patterns_agree(res, outputs, what)
    if anchor and direction == 'forward':
        zy, ld = res['N']
        e = _err(zy.cpu().numpy(), zy_ref)
        print(f'{what}: zy rel err {e:.3e}')
        assert e < RTOL
        check_logdet(ld.cpu().numpy(), ld_ref, abs_s, what)
    elif anchor:
        e = _err(res['N'][0].cpu().numpy(), xy)
        print(f'{what}: inverse rel err {e:.3e}')
        assert e < RTOL


# ---------------------------------------------------------------------------------------------
# 2. per coupling layer
# ---------------------------------------------------------------------------------------------

def _layer_tag(flow, layer):
    info = _lib.cnf_layer_info()
    _lib.check(_lib.load().cnf_plan_layer_info(flow._plan, layer._layer, C.byref(info)), 'layer info')
    return f'layer {layer._layer} (coupling {info.coupling_index}, block {info.block}, {info.h}x{info.w}, fused_net={info.fused_net})'


@pytest.mark.parametrize('name,B,options', [('cfg2', 17, None), ('cfg4', 6, None), ('cfg5', 2, None),
                                            ('cfg4', 6, {'GENERIC': 0}), ('cfg5', 2, {'GENERIC': 0})],
                         ids=['cfg2-B17', 'cfg4-B6', 'cfg5-B2', 'cfg4-B6-GENERIC0', 'cfg5-B2-GENERIC0'])
def test_coupling_layers_ignore_workspace_contents(gpu, name, B, options):
    """Every coupling layer's forward_and_Jacobian / backward at its input of the layer-by-layer walk, under N
    and L against Z: the assertion names every layer whose v, log-det or u_back is not bit-equal."""
    flow, ora, P, xy = _setup(name, B, options=options)
    nbytes = _ws_bytes(flow, B)
    zeros = torch.zeros(B, device=gpu)

    def walk(x, ws, fill):
        """[(layer, u, v, log-det, u_back)] per coupling layer; fill: the workspace byte before every call (None: leave it)"""
        u, zy, out = x, None, []
        for layer in flow.layers_list:
            if hasattr(layer, 'coupling_index'):
                if fill is not None:
                    ws.fill_(fill)
                v, s, _ = layer.forward_and_Jacobian(u, zeros, None)
                if fill is not None:
                    ws.fill_(fill)
                ub, _ = layer.backward(v, None)
                out.append((layer, u, v, s, ub))
                u = v
            else:
                u, _, zy = layer.forward_and_Jacobian(u, None, zy)
        return out

    ws, chk = guarded(nbytes, FILL['Z'])
    flow._ws[B] = ws
    ref = walk(torch.from_numpy(xy).to(gpu), ws, FILL['Z'])
    other = walk(_batch(name, B, 11), ws, None)
    chk(f'{name} B={B} [Z] ws')
    bad = []
    for pat in ('N', 'L'):
        ws, chk = guarded(nbytes, FILL[pat])
        flow._ws[B] = ws
        for (layer, u, v, s, ub), (_, u_o, v_o, _, _) in zip(ref, other):
            if pat == 'L':
                layer.forward_and_Jacobian(u_o, zeros, None)
            else:
                ws.fill_(FILL[pat])
            v2, s2, _ = layer.forward_and_Jacobian(u, zeros, None)
            if pat == 'L':
                layer.backward(v_o, None)
            else:
                ws.fill_(FILL[pat])
            ub2, _ = layer.backward(v, None)
            diffs = [(n, max_diff(a, b2)) for n, a, b2 in (('v', v, v2), ('logdet', s, s2), ('u_back', ub, ub2))
                     if not same_bits(a, b2)]
            if diffs:
                bad.append(f'[{pat}] {_layer_tag(flow, layer)}: ' + ', '.join(f'{n} max abs diff {d:.3e}' for n, d in diffs))
        chk(f'{name} B={B} [{pat}] ws')
    for layer, u, v, s, ub in ref:
        assert torch.isfinite(v).all() and torch.isfinite(s).all() and torch.isfinite(ub).all(), _layer_tag(flow, layer)
    assert not bad, f'{name} B={B} {options}: {len(bad)} layer results depend on the workspace contents\n' + '\n'.join(bad)


# ---------------------------------------------------------------------------------------------
# 3. cnf_flow_forward_noise
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,B,noise', [('cfg2', 3, (0.98, 7, 0, 0.01)),
                                          # the first layer is streamed: the preparation runs as a pass of its own
                                          ('cfg4', 1, (0.98, 7, 0))], ids=['cfg2-B3-logit', 'cfg4-B1'])
def test_forward_noise_ignores_workspace_contents(gpu, name, B, noise):
    flow, ora, P, xy = _setup(name, B)
    what = f'{name} B={B} noise={noise}'
    x, x_other = torch.from_numpy(xy).to(gpu), _batch(name, B, 11)
    if len(noise) > 3:   # the logit map takes the raw images in [0, 1]
        for t in (x, x_other):
            t[..., :PRESETS[name].x_d].clamp_(0.0, 1.0)
    outputs = ('zy', 'ld', 'xn')
    res = {}
    for pat in PATTERNS:
        b = Buffers(pat, ws=_ws_bytes(flow, B), zy=x.shape, ld=(B,), xn=x.shape)
        flow._ws[B] = b.ws
        res[pat] = run_pattern(b, outputs, c_noise, (flow, b, x, noise), (flow, b, x_other, noise))
        b.check(what)
    assert_patterns_agree(res, outputs, what)


# ---------------------------------------------------------------------------------------------
# 4. training step
# ---------------------------------------------------------------------------------------------

TRAIN_CASES = [('small', 3, {}), ('small', 3, {'LDS_BWD': 0}), ('small', 3, {'TRAIN_ALT': 1}),
               ('cfg2', 2, {}), ('cfg2', 2, {'LDS_BWD': 0}), ('cfg2', 2, {'TRAIN_SCHED': 6}), ('cfg2', 2, {'TRAIN_ALT': 32}),
               ('cfg2', 2, {'LAYER_NORM': False}), ('narrow', 3, {}),
               # the benched training batch: the sliced LN backward and the multi-unit band partitions exist only here
               ('cfg2', 64, {})]


def _train_flow(name, opts):
    """_setup's flow and weights; LAYER_NORM is a constructor argument, the other names are debug options."""
    opts = dict(opts)
    if 'LAYER_NORM' not in opts:
        return _setup(name, 2, options=opts)[0]
    from arl_conditional_normalizing_flows_amd.make_model import cFlow
    from oracle.cflow_np import OracleCFlow
    kw = dict(PRESETS[name].kwargs(), LAYER_NORM=opts.pop('LAYER_NORM'))
    flow = cFlow(**kw, debug_options=opts)
    flow.set_weights(OracleCFlow(**kw).init_params(0))
    return flow


@pytest.mark.parametrize('name,B,opts', TRAIN_CASES,
                         ids=['-'.join([n, f'B{B}'] + [f'{k}{int(v)}' for k, v in o.items()]) for n, B, o in TRAIN_CASES])
def test_gradients_ignore_workspace_contents(gpu, name, B, opts):
    """flow.gradients (training forward, NLL, backward) with the train workspace and the gradient vector under
    Z, N and L: the four loss terms and the whole gradient bit-equal and finite, guards intact."""
    flow = _train_flow(name, opts)
    what = f'{name} B={B} {opts} gradients'
    x, x_other = _batch(name, B, 6), _batch(name, B, 11)
    nbytes = int(_lib.load().cnf_plan_train_workspace_bytes(flow._plan, B))
    assert nbytes > 0
    res = {}
    for pat in PATTERNS:
        b = Buffers(pat, ws=nbytes, grads=(flow.num_params,))
        flow._ws[('train', B)] = b.ws
        flow._grads = b.grads
        if pat == 'L':
            flow.gradients(x_other)
        g, terms = flow.gradients(x)
        assert g.data_ptr() == b.grads.data_ptr()
        res[pat] = [g.clone(), torch.stack(list(terms))]
        b.check(what)
    assert_patterns_agree(res, ('gradient', 'loss terms'), what)


# ---------------------------------------------------------------------------------------------
# 5. graph replay
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,B', [('small', 3), ('cfg2', 17)])
def test_graph_replay_equals_eager(gpu, name, B):
    """cnf_flow_forward + cnf_nll + cnf_flow_inverse captured on a side stream into one graph over static buffers
    (after one eager call there: the table upload and the cnf_nll slot, include/cnf.h): the replay equals the
    eager results bit for bit, and so does a replay after another batch was copied into the static input
    and the workspace filled with 0xFF: nothing of capture time is baked in."""
    flow, ora, P, xy = _setup(name, B)
    lib = _lib.load()
    names = ('zy', 'ld', 'per', 'sums', 'xy')
    batches = [torch.from_numpy(xy).to(gpu), _batch(name, B, 11)]
    eager = []
    for x in batches:
        zy, ld = flow(x, 1, per_image_logdet=True)
        sums, per = flow.nll_sums(x, zy, ld)
        eager.append([zy, ld, per, sums, flow(zy, -1)])
    torch.cuda.synchronize()
    b = Buffers('Z', ws=_ws_bytes(flow, B), zy=xy.shape, ld=(B,), per=(B, 3), sums=(4,), xy=xy.shape)
    flow._ws[B] = b.ws
    x_static = batches[0].clone()

    def step():
        c_forward(flow, b, x_static)
        _lib.check(lib.cnf_nll(flow._plan, x_static.data_ptr(), b.zy.data_ptr(), b.ld.data_ptr(), b.per.data_ptr(),
                               b.sums.data_ptr(), B, _st()), 'cnf_nll')
        c_inverse(flow, b, b.zy)

    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step()
    torch.cuda.synchronize()
    for k, x in enumerate(batches):
        with torch.cuda.stream(side):
            if k:
                x_static.copy_(x)
            for n in ('ws',) + names:
                b.raw[n].fill_(0xFF if k else 0x00)
            graph.replay()
        b.check(f'{name} B={B} replay {k}')
        for n, e in zip(names, eager[k]):
            got = getattr(b, n)
            assert torch.isfinite(got).all(), (k, n)
            assert same_bits(got, e), f'{name} B={B} replay {k}: {n} differs from the eager call, max abs diff {max_diff(got, e):.3e}'
    del graph
