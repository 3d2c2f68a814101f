"""The generative direction's log-density: cnf_flow_inverse_logdet / cnf_coupling_inverse_logdet
(cFlow.call(zy, -1, inverse_logdet=True)) and cnf_flow_sample_logp (cFlow.sample(return_log_prob=True)),
include/cnf.h.

CPU part (host only): the argument errors are CNF_E_INVALID before any HIP call, the dry-run schedule of
direction -2 is direction -1's plus at most one k_ld_reduce, and no workspace grew.

GPU part: -logdet of the inverse against the float64 oracle's forward log-det under the project's bound
1e-5 * max(|ref|, sum|s|) (the float64 flow inverts to 1e-12, so the inverse's s are the forward's at xy),
at initialisation for every kernel that writes log-det slots and on a trained-like weight set; xy keeps the
plain inverse's bits; the layer-by-layer walk equals the fused call; nothing depends on the workspace's
contents, the stream, graph replay or the batch an image rides in; log_prob composes from the documented zy
and the inverse's log-det within one fp32 ulp, does not depend on chunk, and agrees with the float64 oracle.

_setup / check_logdet / _err are tests/test_gpu_parity.py's, the trained weight set is
tests/test_value_regimes.py's 'trained' regime, restated here."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from arl_conditional_normalizing_flows_amd import _lib
from arl_conditional_normalizing_flows_amd.config import PRESETS
from oracle.cflow_np import OracleCFlow, synthetic_class_batch, synthetic_sr_batch

RTOL = 1e-5
LOG_2PI = float(np.log(2.0 * np.pi))
KNOBS = {'nogc': {'NETLDS': 0, 'GC': 0}, 'conv1': {'NETLDS': 0, 'PW': 0}}
ALL_PRESETS = ['tiny', 'small', 'cfg2', 'cfg3', 'ref_default', 'cfg4', 'cfg5', 'narrow']


# ---------------------------------------------------------------------------------------------
# CPU: the C ABI's host side
# ---------------------------------------------------------------------------------------------

A, Bp, WS, OUT = 1 << 40, 2 << 40, 3 << 40, 4 << 40   # placeholder device addresses, never dereferenced


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


def _desc(S=4, chunk=3, T=1.0, seed=0, offset=0, logit_a=0.0, residual=0):
    return _lib.cnf_sample_desc(S, chunk, T, seed, offset, logit_a, residual)


def _coupling_layer(lib, p):
    info = _lib.cnf_layer_info()
    for li in range(lib.cnf_plan_num_layers(p)):
        assert lib.cnf_plan_layer_info(p, li, C.byref(info)) == 0
        if info.kind == 0:
            return li
    raise AssertionError('no coupling layer')


def test_argument_errors(lib):
    """CNF_E_INVALID with a message and nothing launched (no GPU is needed): a NULL log-det, xy == zy, a
    non-coupling layer or u == v for the per-layer call, cnf_flow_sample_logp without any output."""
    rc, p, keep = _plan(lib, _capi_kw('tiny'))
    assert rc == 0, lib.cnf_last_error()
    try:
        assert lib.cnf_flow_inverse_logdet(p, A, A, Bp, OUT, None, WS, 2, None) == -1
        assert lib.cnf_last_error()
        assert lib.cnf_flow_inverse_logdet(p, A, A, Bp, Bp, OUT, WS, 2, None) == -1
        assert b'alias' in lib.cnf_last_error()
        assert lib.cnf_flow_inverse_logdet(p, A, A, None, OUT, OUT + (1 << 30), WS, 2, None) == -1
        assert lib.cnf_flow_inverse_logdet(p, A, A, Bp, OUT, OUT + (1 << 30), WS, 0, None) == -1
        li = _coupling_layer(lib, p)
        assert lib.cnf_coupling_inverse_logdet(p, li, A, A, Bp, Bp, OUT, WS, 2, None) == -1
        assert b'alias' in lib.cnf_last_error()
        assert lib.cnf_coupling_inverse_logdet(p, -1, A, A, Bp, OUT, OUT + (1 << 30), WS, 2, None) == -1
        assert b'coupling layer' in lib.cnf_last_error()
        d = _desc()
        assert lib.cnf_flow_sample_logp(p, A, A, Bp, C.byref(d), None, None, None, None, None, WS, 2, None) == -1
        msg = lib.cnf_last_error().decode()
        assert 'output' in msg and 'log_prob' in msg, msg
        assert lib.cnf_flow_sample_logp(p, A, A, None, C.byref(d), None, None, None, None, OUT, WS, 2, None) == -1
        assert 'y' in lib.cnf_last_error().decode()
        bad = _desc(S=0)
        assert lib.cnf_flow_sample_logp(p, A, A, Bp, C.byref(bad), None, None, None, None, OUT, WS, 2, None) == -1
        assert 'num_samples' in lib.cnf_last_error().decode()
    finally:
        lib.cnf_plan_destroy(p)


def test_log_prob_alone_is_an_output(lib):
    """log_prob as the only output passes cnf_plan_sample_workspace_bytes and the argument check. Where no
    device exists the call then stops at its first HIP call (CNF_E_HIP, not CNF_E_INVALID) with placeholder
    addresses untouched; on a device it runs, on real buffers."""
    rc, p, keep = _plan(lib, _capi_kw('tiny'))
    assert rc == 0, lib.cnf_last_error()
    try:
        d = _desc(S=3, chunk=2)
        nbytes = int(lib.cnf_plan_sample_workspace_bytes(p, 2, C.byref(d)))
        assert nbytes > 0
        if not torch.cuda.is_available():
            rc = lib.cnf_flow_sample_logp(p, A, A, Bp, C.byref(d), None, None, None, None, OUT, WS, 2, None)
            msg = lib.cnf_last_error().decode()
            assert rc == -2 and 'output' not in msg, (rc, msg)
            return
        H, W, D = PRESETS['tiny'].io_shape
        x_d = PRESETS['tiny'].x_d
        dev = torch.device('cuda', 0)
        n = int(lib.cnf_plan_num_params(p))
        params = torch.zeros(n, device=dev)
        aux = torch.zeros(int(lib.cnf_plan_aux_floats(p)), device=dev)
        st = torch.cuda.current_stream().cuda_stream
        assert lib.cnf_pack_params(p, params.data_ptr(), aux.data_ptr(), st) == 0
        y = torch.zeros((2, H, W, D - x_d), device=dev)
        ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        lp = torch.full((2, 3), float('nan'), device=dev)
        rc = lib.cnf_flow_sample_logp(p, params.data_ptr(), aux.data_ptr(), y.data_ptr(), C.byref(d), None, None,
                                      None, None, lp.data_ptr(), ws.data_ptr(), 2, st)
        assert rc == 0, lib.cnf_last_error()
        torch.cuda.synchronize()
        assert torch.isfinite(lp).all()   # (zero weights: s = 0, log_prob = log N(z; 0, I))
    finally:
        lib.cnf_plan_destroy(p)


def _schedule(lib, p, B, direction):
    lib.cnf_debug_schedule.restype = C.c_int
    lib.cnf_debug_schedule.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_int]
    buf = C.create_string_buffer(1 << 16)
    n = lib.cnf_debug_schedule(p, B, direction, buf, 1 << 16)
    assert n > 0, lib.cnf_last_error()
    names = buf.value.decode().split('\n')[:-1]
    assert len(names) == n
    return names


@pytest.mark.parametrize('name', ALL_PRESETS)
def test_schedule_with_logdet_is_the_inverse_plus_one_reduce(lib, name):
    """direction -2 (cnf_flow_inverse_logdet) lists direction -1's launches in the same order, plus at most one
    more launch, named k_ld_reduce: the slots are written by the kernels that apply the laws anyway."""
    rc, p, keep = _plan(lib, _capi_kw(name))
    assert rc == 0, lib.cnf_last_error()
    try:
        inv = _schedule(lib, p, 3, -1)
        ld = _schedule(lib, p, 3, -2)
        assert _schedule(lib, p, 3, -1) == inv   # (the -2 run left nothing behind)
    finally:
        lib.cnf_plan_destroy(p)
    extra = list(ld)
    for n in inv:   # inv is a subsequence of ld, in order
        while extra and extra[0] != n:
            assert extra.pop(0) == 'k_ld_reduce'
        assert extra and extra.pop(0) == n
    assert all(n == 'k_ld_reduce' for n in extra)
    assert len(ld) - len(inv) <= 1 and ld.count('k_ld_reduce') == len(ld) - len(inv) + inv.count('k_ld_reduce')


# cnf_plan_workspace_bytes(B) of the commit before the inverse log-det, B = 1, 3, 64: the log-det slots
# [couplings][B][ld_parts] were part of it already
WORKSPACE_BYTES = {
    'tiny': (16384, 45568, 962560),
    'small': (136704, 409856, 8740864),
    'cfg2': (2060288, 6180864, 131858432),
    'cfg3': (2097152, 6291456, 134217728),
    'ref_default': (1553408, 4655360, 99282944),
    'cfg4': (8522240, 25566720, 545423360),
    'cfg5': (35687424, 107062272, 2283995136),
    'narrow': (18688, 52736, 1112064),
}


@pytest.mark.parametrize('name', ALL_PRESETS)
def test_workspaces_did_not_grow(lib, name):
    """cnf_plan_workspace_bytes is what it was, and cnf_plan_sample_workspace_bytes -- the one size for
    cnf_flow_sample and cnf_flow_sample_logp, with or without log_prob -- is still the inverse workspace of a
    chunk, the two chunk buffers and the statistics state (tests/test_sampling.py's form)."""
    kw = _capi_kw(name)
    H, W, D = kw['io_shape']
    x_d = kw['x_d']
    rc, p, keep = _plan(lib, kw)
    assert rc == 0, lib.cnf_last_error()
    try:
        for B, want in zip((1, 3, 64), WORKSPACE_BYTES[name]):
            assert int(lib.cnf_plan_workspace_bytes(p, B)) == want, (name, B)
            for chunk in (1, 3, 64):
                d = _desc(S=5, chunk=chunk)
                need = int(lib.cnf_plan_workspace_bytes(p, chunk)) + 2 * chunk * H * W * D * 4 + 3 * B * H * W * x_d * 4
                got = int(lib.cnf_plan_sample_workspace_bytes(p, B, C.byref(d)))
                assert need <= got <= need + 4 * 256, (name, B, chunk, got, need)
    finally:
        lib.cnf_plan_destroy(p)


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------

def _setup(name, B, group_mode='reference', seed=0, netlds=True, options=None):
    """netlds: True / False (debug option NETLDS), or a KNOBS key (streamed layers with fallback kernels)"""
    from arl_conditional_normalizing_flows_amd.make_model import cFlow
    opt = dict(KNOBS.get(netlds, {'NETLDS': 0 if netlds is False else 1}))
    opt.update(options or {})
    cfg = PRESETS[name]
    kw = cfg.kwargs()
    kw['group_mode'] = group_mode
    flow = cFlow(**kw, debug_options=opt)
    ora = OracleCFlow(**kw)
    P = ora.init_params(seed)
    flow.set_weights(P)
    return flow, ora, P, _batch(name, B, seed + 1)


def _batch(name, B, seed):
    cfg = PRESETS[name]
    H, W, _D = cfg.io_shape
    if cfg.data == 'class':
        return synthetic_class_batch(B, H, W, cfg.x_d, seed=seed)
    return synthetic_sr_batch(B, H, W, cfg.x_d, cfg.sr_pow, seed=seed)


def ld_tol(ld_ref, abs_s):
    """per-image log-det bound of the project: 1e-5 * max(|ref|, sum|s|)."""
    return RTOL * np.maximum(np.abs(np.asarray(ld_ref, np.float64)), np.asarray(abs_s, np.float64))


def check_logdet(ld_gpu, ld_ref, abs_s, what=''):
    e = np.abs(np.asarray(ld_gpu, np.float64) - np.asarray(ld_ref, np.float64))
    tol = ld_tol(ld_ref, abs_s)
    print(f'{what} logdet: max abs err {e.max():.3e}, worst err/tol {np.max(e / tol):.3f} '
          f'(|ref| <= {np.abs(ld_ref).max():.3e}, sum|s| >= {np.min(abs_s):.3e})')
    assert np.all(e <= tol), (e, tol)


def _err(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# every slot writer: k_map2 and one slot per image (tiny); k_net_lds comp / tail paths and k_coupling (small, cfg2,
# ref_default, cfg4, cfg5); k_coupling per layer, also in tap mode and after the fallback kernels (streamed,
# nogc, conv1); couplings 1 and 2 pixels wide (narrow)
PARITY = [('tiny', 2, True), ('small', 3, True), ('small', 3, False), ('cfg2', 2, True), ('cfg2', 2, False),
          ('cfg2', 2, 'nogc'), ('small', 3, 'conv1'), ('narrow', 3, True), ('narrow', 3, False),
          ('ref_default', 2, True), ('cfg4', 2, True), ('cfg5', 1, True)]


@pytest.mark.gpu
@pytest.mark.parametrize('name,B,netlds', PARITY)
def test_inverse_logdet_matches_oracle(gpu, name, B, netlds):
    """x within 1e-5 of xy and -logdet within 1e-5 * max(|ld_ref|, sum|s|) of the float64 forward log-det at
    xy. Measured worst err/tol over the cases: see DESIGN.md (inverse log-det)."""
    flow, ora, P, xy = _setup(name, B, netlds=netlds)
    zy_ref, ld_ref, abs_s = ora.forward(xy, P, abs_s=True)
    x, ld = flow(torch.from_numpy(zy_ref.astype(np.float32)).to(gpu), -1, inverse_logdet=True)
    torch.cuda.synchronize()
    assert ld.shape == (B,) and ld.dtype == torch.float32
    e = _err(x.cpu().numpy(), xy)
    print(f'{name} lds={netlds}: inverse rel err {e:.3e}')
    assert e < RTOL
    check_logdet(-ld.cpu().numpy().astype(np.float64), ld_ref, abs_s, f'{name} lds={netlds} inverse')


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


@pytest.mark.gpu
@pytest.mark.parametrize('name,netlds', [('small', True), ('small', False)])
def test_inverse_logdet_away_from_initialisation(gpu, name, netlds):
    """Trained-like weights (saturating s): the reference is the float64 forward of the GPU's own x, so the
    inverse's ill-conditioning does not enter; the bound is the same."""
    flow, ora, P0, xy = _setup(name, 3, seed=2, netlds=netlds)
    P = _trained(ora.init_params(2))
    flow.set_weights(P)
    zy = ora.forward(xy, P)[0].astype(np.float32)
    x, ld = flow(torch.from_numpy(zy).to(gpu), -1, inverse_logdet=True)
    torch.cuda.synchronize()
    assert torch.isfinite(x).all() and torch.isfinite(ld).all()
    _, ld_ref, abs_s = ora.forward(x.cpu().numpy().astype(np.float64), P, abs_s=True)
    check_logdet(-ld.cpu().numpy().astype(np.float64), ld_ref, abs_s, f'{name} lds={netlds} trained inverse')


LAYERWISE = [('tiny', 2), ('small', 3), ('cfg2', 2), ('ref_default', 2), ('cfg3', 5), ('cfg4', 3), ('cfg5', 1)]


@pytest.mark.gpu
@pytest.mark.parametrize('name,B', LAYERWISE)
def test_xy_bits_and_layerwise_equals_fused(gpu, name, B):
    """x of inverse_logdet=True is the plain inverse's bit for bit (fused and layer by layer), and the
    layer-by-layer log-det (a k_coupling and a reduction per layer, accumulated in fp32) agrees with the fused
    one as the forward's does (test_layerwise_equals_fused: rtol 1e-6, atol 1e-5)."""
    flow, ora, P, xy = _setup(name, B)
    zy = flow(torch.from_numpy(xy).to(gpu), 1)[0]
    x0 = flow(zy, -1)
    x1, ld1 = flow(zy, -1, inverse_logdet=True)
    x2, ld2 = flow(zy, -1, inverse_logdet=True, layerwise=True)
    torch.cuda.synchronize()
    assert torch.equal(x1, x0) and torch.equal(x2, x0)
    assert torch.isfinite(ld1).all()
    assert torch.allclose(ld1, ld2, rtol=1e-6, atol=1e-5), (ld1, ld2)
    # the per-layer entry point alone: logdet_accum -= the layer's sum, NULL skips it
    layer = next(L for L in flow.layers_list if hasattr(L, 'backward_and_Jacobian'))
    torch.manual_seed(3)
    v = torch.randn(B, layer.input_height, layer.input_width, layer.input_depth, device=gpu)
    u0, _ = layer.backward(v, None)
    u1, acc, z = layer.backward_and_Jacobian(v, torch.full((B,), 2.0, device=gpu), None)
    v2, fwd, _ = layer.forward_and_Jacobian(u1, torch.zeros(B, device=gpu), None)
    assert z is None and torch.equal(u1, u0)
    # the forward at u1 sees the same conditioning half: the same s, the opposite sign
    assert torch.allclose(acc - 2.0, -fwd, rtol=1e-6, atol=1e-5)


def c_inverse_logdet(flow, z, xy, ld, ws=None):
    B = z.shape[0]
    ws = flow._workspace(B) if ws is None else ws
    _lib.check(_lib.load().cnf_flow_inverse_logdet(flow._plan, flow.params.data_ptr(), flow._aux.data_ptr(),
                                                   z.data_ptr(), xy.data_ptr(), ld.data_ptr(), ws.data_ptr(), B,
                                                   torch.cuda.current_stream().cuda_stream), 'cnf_flow_inverse_logdet')


@pytest.mark.gpu
@pytest.mark.parametrize('name,B,netlds', [('cfg2', 7, True), ('cfg2', 7, False), ('small', 3, True), ('tiny', 3, True)])
def test_state_independence(gpu, name, B, netlds):
    """(x, logdet) bit-equal after the workspace was filled with 0xFF bytes (every slot a NaN), after a forward
    on the same workspace (its slots hold the forward's sums of another batch), on a non-default stream and
    under graph replay; and logdet[:3] of the batch equals the call on its first 3 images."""
    flow, ora, P, xy = _setup(name, B, netlds=netlds)
    z = flow(torch.from_numpy(xy).to(gpu), 1)[0]
    x0, ld0 = flow(z, -1, inverse_logdet=True)
    torch.cuda.synchronize()
    assert torch.isfinite(ld0).all()

    def check(what, x, ld):
        torch.cuda.synchronize()
        assert same_bits(x, x0), f'{name} {what}: x differs'
        assert same_bits(ld, ld0), f'{name} {what}: logdet differs ({ld} vs {ld0})'

    flow._workspace(B).fill_(0xFF)
    check('NaN workspace', *flow(z, -1, inverse_logdet=True))
    flow(torch.from_numpy(_batch(name, B, 11)).to(gpu), 1)
    check('after a forward', *flow(z, -1, inverse_logdet=True))
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        xs, lds = flow(z, -1, inverse_logdet=True)
    side.synchronize()
    check('side stream', xs, lds)
    # graph replay over static buffers (cnf_pack_params ran in set_weights; one eager call on the stream first)
    xg, ldg = torch.empty_like(x0), torch.empty_like(ld0)
    with torch.cuda.stream(side):
        c_inverse_logdet(flow, z, xg, ldg)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        c_inverse_logdet(flow, z, xg, ldg)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        flow._workspace(B).fill_(0xFF)
        xg.fill_(float('nan'))
        ldg.fill_(float('nan'))
        graph.replay()
    check('graph replay', xg, ldg)
    del graph
    x3, ld3 = flow(z[:3].contiguous(), -1, inverse_logdet=True)
    torch.cuda.synchronize()
    assert same_bits(x3, x0[:3]) and same_bits(ld3, ld0[:3]), f'{name}: the first 3 images alone differ'


# ---- sampling --------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _sflow(name):
    flow, ora, P, xy = _setup(name, 3)
    x_d = PRESETS[name].x_d
    y = torch.from_numpy(np.ascontiguousarray(xy[..., x_d:])).cuda()
    return flow, ora, P, y


def _zy_kw(kw, y, S, T, seed, offset):
    """the documented latent of a flow built from kw: renew_noise of [B,S,H,W,x_d], times T, concatenated with y"""
    from arl_conditional_normalizing_flows_amd.base_functions import renew_noise
    H, W, D = kw['io_shape']
    B, x_d = y.shape[0], kw['x_d']
    z = renew_noise(torch.empty((B, S, H, W, x_d), device=y.device), seed=seed, offset=offset)
    yb = y[:, None].expand(B, S, H, W, D - x_d)
    return torch.cat([T * z, yb], dim=-1).reshape(B * S, H, W, D).contiguous()


def _zy(name, y, S, T, seed, offset):
    return _zy_kw(PRESETS[name].kwargs(), y, S, T, seed, offset)


def _composed_kw(kw, flow, zy, B, S):
    """(expected fp32 log_prob, the one-ulp bound) [B,S] from the documented zy and the inverse's log-det"""
    x_d = kw['x_d']
    ld = flow(zy, -1, inverse_logdet=True)[1].cpu().numpy().astype(np.float64)
    z = zy[..., :x_d].cpu().numpy().astype(np.float64).reshape(B * S, -1)
    llz = -0.5 * (z * z).sum(axis=1) - 0.5 * z.shape[1] * LOG_2PI
    expected = (llz - ld).astype(np.float32)
    bound = np.spacing((np.abs(llz) + np.abs(ld)).astype(np.float32))
    return expected.reshape(B, S), bound.reshape(B, S).astype(np.float64)


def _composed(name, flow, zy, B, S):
    return _composed_kw(PRESETS[name].kwargs(), flow, zy, B, S)


def log_prob_oracle(ora, P, zy, x_d):
    """float64 log_prob of the draws whose latent is zy [n,H,W,D] (numpy) and its bound: the oracle's inverse,
    its forward log-det there, log N(z; 0, I); 1e-5 of the conditioning scale max(|llz| + |ld_ref|,
    0.5 sum z^2 + sum|s|), the form of the NLL parity test. Returns (ref [n], tol [n])."""
    x64 = ora.inverse(zy, P)
    _, ld_ref, abs_s = ora.forward(x64, P, abs_s=True)
    z = zy[..., :x_d].astype(np.float64).reshape(len(zy), -1)
    q = (z * z).sum(axis=1)
    llz = -0.5 * q - 0.5 * z.shape[1] * LOG_2PI
    return llz + ld_ref, RTOL * np.maximum(np.abs(llz) + np.abs(ld_ref), 0.5 * q + abs_s)


@pytest.mark.gpu
@pytest.mark.parametrize('T', [1.0, 0.7])
@pytest.mark.parametrize('name', ['tiny', 'small', 'cfg2'])
def test_log_prob_composes_from_zy_and_the_inverse_logdet(gpu, name, T):
    """log_prob == float32(-0.5 sum z^2 - 0.5 n log(2 pi) - logdet) of the documented zy and
    call(zy, -1, inverse_logdet=True)[1], within one fp32 ulp at |llz| + |ld| (the fp32 rounding of ld in the C
    call and the final rounding)."""
    flow, ora, P, y = _sflow(name)
    B, S = 3, 5
    zy = _zy(name, y, S, T, seed=5, offset=3)
    expected, bound = _composed(name, flow, zy, B, S)
    out = flow.sample(y, S, temperature=T, seed=5, offset=3, return_samples=False, return_stats=False,
                      return_log_prob=True)
    assert sorted(out) == ['log_prob'] and out['log_prob'].shape == (B, S)
    got = out['log_prob'].cpu().numpy()
    assert np.isfinite(got).all()
    d = np.abs(got.astype(np.float64) - expected.astype(np.float64))
    print(f'{name} T={T}: worst |log_prob - expected| / bound {np.max(d / bound):.3f}')
    assert np.all(d <= bound), (d, bound)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['tiny', 'small', 'cfg2'])
def test_log_prob_does_not_depend_on_chunk(gpu, name):
    """log_prob bit-equal for chunk in {1, 4, 7, B S, 64} (B = 3, S = 5: chunks straddle conditions), and
    samples, mean, std, y_dev bit-equal to a call without log_prob."""
    flow, ora, P, y = _sflow(name)
    B, S = 3, 5
    kw = dict(temperature=0.9, seed=7, offset=2, return_y_dev=True)
    plain = flow.sample(y, S, chunk=4, **kw)
    ref = None
    for chunk in (1, 4, 7, B * S, 64):
        got = flow.sample(y, S, chunk=chunk, return_log_prob=True, **kw)
        assert sorted(got) == ['log_prob', 'mean', 'samples', 'std', 'y_dev']
        assert torch.isfinite(got['log_prob']).all()
        ref = got if ref is None else ref
        assert same_bits(got['log_prob'], ref['log_prob']), f'{name} chunk={chunk}: log_prob differs'
        for n, t in plain.items():
            assert same_bits(got[n], t), f'{name} chunk={chunk}: {n} differs from the call without log_prob'
    # the draws of a condition are not all equally probable
    assert (ref['log_prob'].max(dim=1).values > ref['log_prob'].min(dim=1).values).all()


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['tiny', 'small', 'cfg2'])
def test_log_prob_at_temperature_zero(gpu, name):
    """T = 0: every draw of a condition is the same image, so its S values are bit-identical, and equal
    float32(-0.5 n log(2 pi) - ld) within the composition bound."""
    flow, ora, P, y = _sflow(name)
    B, S = 3, 5
    zy = _zy(name, y, S, 0.0, seed=1, offset=0)
    expected, bound = _composed(name, flow, zy, B, S)
    got = flow.sample(y, S, temperature=0.0, seed=1, chunk=4, return_stats=False, return_log_prob=True)['log_prob']
    assert torch.isfinite(got).all()
    for b in range(B):
        assert same_bits(got[b], got[b, :1].expand(S)), (b, got[b])
    d = np.abs(got.cpu().numpy().astype(np.float64) - expected.astype(np.float64))
    assert np.all(d <= bound), (d, bound)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['tiny', 'small'])
def test_log_prob_matches_oracle(gpu, name):
    """The whole against float64: the oracle's inverse of the documented zy (the latent read back from the
    device), its forward log-det there, log N(z; 0, I) in float64. Bound: 1e-5 of the conditioning scale
    max(|llz| + |ld_ref|, 0.5 sum z^2 + sum|s|), the form of the NLL parity test."""
    flow, ora, P, y = _sflow(name)
    B, S, x_d = 3, 5, PRESETS[name].x_d
    zy = _zy(name, y, S, 1.0, seed=4, offset=0).cpu().numpy()
    ref, tol = log_prob_oracle(ora, P, zy, x_d)
    got = flow.sample(y, S, seed=4, return_samples=False, return_stats=False,
                      return_log_prob=True)['log_prob'].cpu().numpy().astype(np.float64).reshape(-1)
    e = np.abs(got - ref)
    print(f'{name}: log_prob max abs err {e.max():.3e}, worst err/tol {np.max(e / tol):.3f}')
    assert np.all(e <= tol), (e, tol)
