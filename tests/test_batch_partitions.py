"""The training backward across batch sizes: every way it partitions the batch, at a ragged edge.

Every other gradient test runs at B = 2 or 3 (plus cfg2 at B = 64, where everything divides evenly), and at
those sizes each partition below is degenerate: k_lnb_apply's 8 batch slices, k_wgrad_direct's row bands per
image, k_wgrad_thin's images per workgroup, k_wgrad_band's unit loop, the VALU k_wgrad's pixel chunks,
k_tconv_band's SUB > 1 tiles (chosen from a workgroup count that includes B), the chunk loop of
k_grad_scatter and the image loop of k_grad_rows beyond one trip, and the training forward's k_pw with several
images per workgroup. They share wpart / lnpart / rows scratch between chunks and slices, so a wrong bound
drops or doubles an image, reads a slot nobody wrote, or writes past a partial-row block.

CASES holds, per edge, the smallest (row, B, debug options) found to reach it. Rows are presets, rows of
test_shape_sweep.SWEEP, or ONE16. Weights are init_params(5), inputs default_rng(6).standard_normal, as in the
sweep's gradient tests.

CPU part (against the cross-compiled library, no GPU):
  test_coverage_claims   what each case is said to reach, from the host functions the launch code itself calls
                         (cnf_debug_train_convs / _wgrad_choice / _tconv_choice / _lnb_slicing /
                         _grad_rows_trips / _pw_ipw)
  test_a_lost_image_is_visible   the bar can see one lost image: the float64 gradient with one image's
                         contribution removed (still divided by B) moves, in every coupling layer, a
                         convolution kernel and a LayerNorm gamma by at least SENSITIVITY x that tensor's
                         tolerance, for three probe images. Where plain inputs do not give that (large B: one
                         image is 1 / B of the mean), the probe images are scaled by PROBE_SCALE.

GPU part: flow.gradients with the train workspace and the gradient vector between test_state_independence's
guard bands, under fill patterns N and Z: finite, bit-equal, guards intact; the N result against float64
autograd under test_train's bar and loss-term bound (check_gradients, imported with its constants)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from arl_conditional_normalizing_flows_amd import _lib
from arl_conditional_normalizing_flows_amd.config import PRESETS
from oracle.cflow_np import OracleCFlow

from test_capi import _plan
from test_shape_sweep import SWEEP, _kw, _opt_str, _row
from test_train import PERTURB, PERTURB_LARGE_B, PERTURB_SEEDS, _tol, check_gradients, oracle_grads

# one block of two coupling layers on 16x16 and two on 8x8, nothing else: the cheapest flow whose 16x16 data
# gradients reach 256 workgroups of 64 * 4 pixels
ONE16 = _row((16, 16, 4), 3, (0,), (1,), (16,), (4,))

# (row, B, debug options), in the order the GPU cases run
CASES = [
    ('small', 1, {}), ('small', 1, {'LDS_BWD': 0}),
    ('small', 9, {}), ('small', 9, {'LDS_BWD': 0}), ('small', 9, {'LDS_BWD': 0, 'TRAIN_ALT': 1}),
    ('small', 85, {}), ('small', 85, {'NETLDS': 0}),
    ('tall', 129, {'NETLDS': 0}),
    ('one16', 256, {'NETLDS': 0}),
    ('nk24', 128, {'NETLDS': 0}),
    ('tiny', 257, {}), ('tiny', 257, {'NETLDS': 0}),
    ('w12x20', 257, {'NETLDS': 0}),
    ('w2', 37, {'LDS_BWD': 0}),
    ('min4x4', 2049, {'NETLDS': 0}),
]
IDS = ['-'.join([r, f'B{B}'] + [f'{k}{v}' for k, v in o.items()]) for r, B, o in CASES]
ROW_BATCHES = sorted({(r, B) for r, B, _ in CASES}, key=[(r, B) for r, B, _ in CASES].index)

SENSITIVITY = 4.0   # a lost image moves a tensor by at least this many tolerances: well clear of the bar
# factor on the probe images' inputs, chosen on the CPU as the smallest power of two at which the float64
# reference alone meets the sensitivity condition (1 where plain standard-normal inputs do)
PROBE_SCALE = {('small', 9): 4.0, ('small', 85): 8.0, ('tall', 129): 8.0, ('one16', 256): 16.0, ('nk24', 128): 8.0,
               ('tiny', 257): 16.0, ('w12x20', 257): 16.0, ('w2', 37): 2.0, ('min4x4', 2049): 32.0}

# (row, B) whose bar has test_train's perturbation term: the cases that fail without it through LeakyReLU kink
# flips alone (the float64 gradient's own spread under PERTURB exceeds the error; figures in DESIGN.md)
PERTURB_CASES = {('nk24', 128)}

# kernel codes of cnf_debug_wgrad_choice / cnf_debug_tconv_choice (WGradKernel, TConvKernel in cnf_kernels.h)
W_VALU, W_THIN, W_DIRECT, W_BAND = range(4)
T_VALU, T_THIN, T_BAND, T_MFMA = range(4)
ROLES = ('conv_out', 'conv_b', 'branch', 'conv_a', 'conv_in')


def kw_of(row):
    """constructor arguments of cFlow / OracleCFlow / TorchCPUFlow"""
    if row in PRESETS:
        return PRESETS[row].kwargs()
    return dict(ONE16, group_mode='reference') if row == 'one16' else _kw(row)


def lnb_slice(B):
    """(slices, images per slice) of the LN backward (only used to pick a probe image; the claims read the library)"""
    S = min(B, 8)
    return S, -(-B // S)


def probes(B):
    """the probe images: image 0, the first image of the last non-empty LN-backward slice, the last image"""
    _, bs = lnb_slice(B)
    return sorted({0, (B - 1) // bs * bs, B - 1})


def inputs(row, B):
    H, W, D = kw_of(row)['io_shape']
    xy = np.random.default_rng(6).standard_normal((B, H, W, D)).astype(np.float32)
    f = PROBE_SCALE.get((row, B), 1.0)
    if f != 1.0:
        xy[probes(B)] *= np.float32(f)
    return xy


@functools.lru_cache(maxsize=None)
def _refs(row, B):
    """float64 and fp32 autograd of a (row, B), computed once (shared by the options and by both parts)"""
    kw = kw_of(row)
    xy = inputs(row, B)
    xy.setflags(write=False)
    P = OracleCFlow(**kw).init_params(5)   # check_gradients' weights
    G_ref, terms_ref = oracle_grads(kw, P, xy)
    G32, _ = oracle_grads(kw, P, xy, torch.float32)
    for g in list(G_ref.values()) + list(G32.values()):
        g.setflags(write=False)
    return kw, P, xy, (G_ref, terms_ref, G32)


# ---------------------------------------------------------------------------------------------
# CPU: coverage
# ---------------------------------------------------------------------------------------------

class Part:
    """one launch's partition as the library reports it"""

    def __init__(self, **kv):
        self.__dict__.update(kv)

    def __repr__(self):
        return 'Part(' + ', '.join(f'{k}={v}' for k, v in self.__dict__.items()) + ')'


def _words(fn, n, *args):
    buf = (C.c_int * n)()
    got = fn(*args, buf, n)
    assert got > 0, (fn.__name__, args, _lib.load().cnf_last_error())
    return list(buf[:got])


def partitions(lib, row, B, opts):
    """Per coupling layer of the case's plan: lds_bwd (the fused k_lds_bwd + k_grad_rows) or, of the multi-kernel
    backward, every convolution's weight-gradient and data-gradient launch and the LN backward's slicing; and
    the forward's k_pw launches."""
    kw = {k: v for k, v in kw_of(row).items() if k != 'group_mode'}
    rc, p, keep = _plan(lib, kw, options=_opt_str(opts))
    assert rc == 0, lib.cnf_last_error()
    try:
        layers = []
        info = _lib.cnf_layer_info()
        for li in range(lib.cnf_plan_num_layers(p)):
            assert lib.cnf_plan_layer_info(p, li, C.byref(info)) == 0
            if info.kind != 0:
                continue
            w = _words(lib.cnf_debug_train_convs, 512, p, info.coupling_index)
            lds_bwd, hc, wc, dc1, dc2, nk, gc, R, n = w[:9]
            L = Part(index=info.coupling_index, lds_bwd=bool(lds_bwd), h=hc, w=wc, nk=nk, gc=gc, R=R, wgrad=[], dgrad=[],
                     lnb=[], rows_trips=lib.cnf_debug_grad_rows_trips(B))
            assert (hc, wc, nk) == (info.hc, info.wc, info.num_kernels)
            for i in range(n):
                role, taps, dil, cin, cout, x_cs, x_off, y_cs, y_off = w[9 + 9 * i:18 + 9 * i]
                tag = dict(role=ROLES[role], h=hc, w=wc, taps=taps, dil=dil, cin=cin, cout=cout)
                k = _words(lib.cnf_debug_wgrad_choice, 6, p, hc, wc, taps, dil, cin, cout, x_cs, B)
                L.wgrad.append(Part(kernel=k[0], chunks=k[1], units=k[2], per_chunk=k[3], short_last=bool(k[4]),
                                    scatter_trips=k[5], **tag))
                t = _words(lib.cnf_debug_tconv_choice, 6, p, hc, wc, taps, dil, cin, cout, y_cs, y_off, x_cs, x_off, B)
                L.dgrad.append(Part(kernel=t[0], NR=t[1], SUB=t[2], TH=t[3], bands=t[5], **tag))
            for n_img in (hc * wc * nk, hc * wc * gc) if R > 0 else (hc * wc * nk,):
                s = _words(lib.cnf_debug_lnb_slicing, 4, n_img, B)
                L.lnb.append(Part(S=s[0], bs=s[1], shared=bool(s[2]), last=B - (-(-B // s[1]) - 1) * s[1],
                                  empty=s[0] - -(-B // s[1])))
            layers.append(L)
        nw = lib.cnf_debug_pw_words()
        buf = (C.c_int * (1 << 16))()
        n = lib.cnf_debug_pw_shapes(p, B, buf, 1 << 16)
        assert n >= 0, lib.cnf_last_error()
        pw = []
        for i in range(0, n, nw):
            s = list(buf[i:i + nw])   # PwShape: nr, gm, ln, res, tap, H, W, tiles_per_img, nprob, ...
            pw.append(Part(h=s[5], w=s[6], tiles=s[7], nprob=s[8], ipw=lib.cnf_debug_pw_ipw(s[7], s[8], s[3], B)))
        return layers, pw
    finally:
        lib.cnf_plan_destroy(p)


def _multi(layers):
    """the layers on the multi-kernel backward"""
    return [L for L in layers if not L.lds_bwd]


def _wg(layers, kernel, **match):
    return [g for L in _multi(layers) for g in L.wgrad
            if g.kernel == kernel and all(getattr(g, k) == v for k, v in match.items())]


def _dg(layers, **match):
    return [d for L in _multi(layers) for d in L.dgrad if all(getattr(d, k) == v for k, v in match.items())]


def _ln(layers):
    return [s for L in _multi(layers) for s in L.lnb]


def test_coverage_claims(lib):
    """What DESIGN.md's table says each case reaches, read from the library: a change of a launch heuristic, of
    a row or of the planner that takes a case off its edge fails here, not silently."""
    reach = {(r, B, _opt_str(o)): partitions(lib, r, B, o) for r, B, o in CASES}

    def of(row, B, **opts):
        return reach[(row, B, _opt_str(opts))]

    # B = 1 on both backward paths: one slice, one image per chunk
    L, _ = of('small', 1)
    assert all(x.lds_bwd and x.rows_trips == 1 for x in L)
    L, _ = of('small', 1, LDS_BWD=0)
    assert not any(x.lds_bwd for x in L) and all(s.S == 1 and s.bs == 1 for s in _ln(L))

    # small B = 9: 8 LN slices of 2 images, the last three of them empty
    assert all(x.lds_bwd for x in of('small', 9)[0])
    L, _ = of('small', 9, LDS_BWD=0)
    assert _ln(L) and all((s.S, s.bs, s.last, s.empty, s.shared) == (8, 2, 1, 3, True) for s in _ln(L))
    # ... and with TRAIN_ALT=1 every weight gradient on the VALU k_wgrad: 16x16 layers 2304 px in 5 chunks of 464
    # whose edges fall inside images. (With LDS_BWD at its default every layer of `small` runs the fused k_lds_bwd
    # and TRAIN_ALT=1 reaches no k_wgrad at all: the option pair is what reaches the kernel.)
    L, _ = of('small', 9, LDS_BWD=0, TRAIN_ALT=1)
    assert not any(x.lds_bwd for x in L)
    assert all(g.kernel == W_VALU for x in L for g in x.wgrad)
    assert all(d.kernel == T_VALU for x in L for d in x.dgrad)
    g16 = _wg(L, W_VALU, h=16, w=16)
    assert g16 and all((g.chunks, g.per_chunk, g.short_last) == (5, 464, True) for g in g16)

    # small B = 85: k_grad_rows' second, ragged trip on the default path
    L, _ = of('small', 85)
    assert all(x.lds_bwd and x.rows_trips == 2 for x in L) and 85 % 64 != 0
    # streamed: LN slices of 11 images, the last of 8; k_wgrad_direct row bands of 6 on H = 16 and of 3 on H = 8,
    # the last band short in both; the forward's k_pw with 2 images per workgroup and a one-image tail
    L, pw = of('small', 85, NETLDS=0)
    assert _ln(L) and all((s.S, s.bs, s.last, s.empty) == (8, 11, 8, 0) for s in _ln(L))
    for h, rb in ((16, 6), (8, 3)):
        gs = _wg(L, W_DIRECT, h=h)
        assert gs and all((g.per_chunk, g.units, g.short_last, g.chunks) == (rb, 3, True, 255) for g in gs), (h, gs)
    assert any(q.ipw == 2 for q in pw) and 85 % 2 == 1

    # tall B = 129: k_tconv_band SUB = 2 on 24x8, row bands of 16 then 8; k_wgrad_thin 2 row tiles, 2 images per
    # workgroup, the last group one image; k_wgrad_direct one band per image
    L, _ = of('tall', 129, NETLDS=0)
    ds = _dg(L, kernel=T_BAND, SUB=2, h=24, w=8)
    assert ds and all((d.TH, d.bands, d.NR) == (16, 2, 1) for d in ds) and 24 % 16 == 8
    gs = _wg(L, W_THIN, h=24, w=8)
    assert gs and all((g.units, g.per_chunk, g.short_last, g.chunks) == (2, 2, True, 130) for g in gs)
    gs = _wg(L, W_DIRECT)
    assert gs and all(g.units == 1 and g.chunks == 129 for g in gs)

    # k_tconv_band<1, 4> and <2, 2>
    L, _ = of('one16', 256, NETLDS=0)
    assert _dg(L, kernel=T_BAND, NR=1, SUB=4, h=16, w=16)
    L, _ = of('nk24', 128, NETLDS=0)
    ds = _dg(L, kernel=T_BAND, NR=2, SUB=2)
    assert ds and all(d.cin == 24 for d in ds)

    # tiny B = 257: k_grad_rows 5 trips on the default path; streamed, k_wgrad_direct writes 257 partial rows (more
    # than WGRAD_MAX_CHUNKS = 256) and k_grad_scatter takes a second trip, k_wgrad_thin has 2 images per workgroup
    # and a one-image tail, the LN slices hold 33 images and the last 26
    L, _ = of('tiny', 257)
    assert all(x.lds_bwd and x.rows_trips == 5 for x in L)
    L, _ = of('tiny', 257, NETLDS=0)
    gs = _wg(L, W_DIRECT)
    assert gs and all((g.chunks, g.scatter_trips, g.units) == (257, 2, 1) for g in gs)
    gs = _wg(L, W_THIN)
    assert gs and all((g.per_chunk, g.short_last, g.chunks) == (2, True, 129) for g in gs)
    assert _ln(L) and all((s.S, s.bs, s.last, s.shared) == (8, 33, 26, True) for s in _ln(L))

    # w12x20 B = 257: k_wgrad_band on 6x10 and 3x5 with 257 units over 256 grid columns: the unit loop's second trip
    L, _ = of('w12x20', 257, NETLDS=0)
    for h, w in ((6, 10), (3, 5)):
        gs = _wg(L, W_BAND, h=h, w=w)
        assert gs and all((g.units, g.chunks) == (257, 256) for g in gs), (h, w)

    # w2 B = 37: the VALU k_wgrad (W < 4) on 16x2: 1184 px in 3 chunks of 400 = 12.5 images
    L, _ = of('w2', 37, LDS_BWD=0)
    gs = _wg(L, W_VALU, h=16, w=2)
    assert gs and all((g.chunks, g.per_chunk, g.short_last) == (3, 400, True) for g in gs)
    assert all(g.kernel == W_VALU for x in L for g in x.wgrad)

    # min4x4 B = 2049: LN slices of 257 images, more than k_lnb_apply shares through LDS: the per-thread sums;
    # k_wgrad in 17 chunks
    L, _ = of('min4x4', 2049, NETLDS=0)
    assert _ln(L) and all((s.S, s.bs, s.shared) == (8, 257, False) for s in _ln(L))
    assert any(g.chunks == 17 for g in _wg(L, W_VALU))
    # one image fewer per slice and the sums are shared: the threshold is this case's
    assert _words(lib.cnf_debug_lnb_slicing, 4, 16, 2048)[:3] == [8, 256, 1]


# ---------------------------------------------------------------------------------------------
# CPU: sensitivity
# ---------------------------------------------------------------------------------------------

def lost_image_margins(row, B):
    """{probe image: {coupling: (kernel margin, gamma margin)}}: by how many tolerances the float64 gradient
    without that image's contribution (the rest still divided by B) differs from the whole one, at the best
    convolution kernel and the best LN gamma of each coupling layer. The loss is a mean over images and every
    layer acts per image, so the lost share is the image's own gradient (a batch of one) / B."""
    kw, P, xy, (G_ref, terms_ref, G32) = _refs(row, B)
    assert all(np.isfinite(g).all() for g in G_ref.values()) and all(np.isfinite(g).all() for g in G32.values())
    assert np.isfinite(terms_ref).all()
    gmax = max(float(np.max(np.abs(v))) for v in G_ref.values())
    tol = {n: _tol(np.asarray(G_ref[n]).reshape(-1), np.asarray(G32[n]).reshape(-1), gmax) for n in G_ref}
    out = {}
    for j in probes(B):
        G1, _ = oracle_grads(kw, P, xy[j:j + 1])
        m = {}
        for n, g in G1.items():
            kind = 0 if n.endswith('.kernel') else 1 if n.endswith('.gamma') else None
            if kind is None:
                continue
            c = m.setdefault(n.split('.', 1)[0], [0.0, 0.0])
            c[kind] = max(c[kind], float(np.max(np.abs(g))) / B / tol[n])
        out[j] = {c: tuple(v) for c, v in m.items()}
    return out


@pytest.mark.parametrize('row,B', ROW_BATCHES, ids=[f'{r}-B{B}' for r, B in ROW_BATCHES])
def test_a_lost_image_is_visible(row, B):
    margins = lost_image_margins(row, B)
    worst = min(min(v) for m in margins.values() for v in m.values())
    print(f'{row} B={B} scale {PROBE_SCALE.get((row, B), 1.0)}: probes {sorted(margins)}, smallest per-layer margin '
          f'{worst:.1f} tolerances')
    for j, m in margins.items():
        assert len(m) == sum(1 for e in OracleCFlow(**kw_of(row)).layers if e.kind == 'coupling')
        for c, (mk, mg) in m.items():
            assert mk >= SENSITIVITY and mg >= SENSITIVITY, (row, B, j, c, mk, mg)


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('row,B,opts', CASES, ids=IDS)
def test_gradients_at_batch_edges(gpu, row, B, opts):
    from test_state_independence import Buffers, max_diff, same_bits
    from test_train import _gpu_flow
    kw, P, xy, refs = _refs(row, B)
    flow = _gpu_flow(kw, P, gpu, dict(opts) or None)
    what = f'{row} B={B} {opts}'
    x = torch.from_numpy(xy.copy()).to(gpu)
    nbytes = int(_lib.load().cnf_plan_train_workspace_bytes(flow._plan, B))
    assert nbytes > 0
    res = {}
    for pat in ('Z', 'N'):
        b = Buffers(pat, ws=nbytes, grads=(flow.num_params,))
        flow._ws[('train', B)] = b.ws
        flow._grads = b.grads
        g, terms = flow.gradients(x)
        assert g.data_ptr() == b.grads.data_ptr()
        res[pat] = [g.clone(), torch.stack(list(terms))]
        b.check(what)
    for n, z, nn in zip(('gradient', 'loss terms'), res['Z'], res['N']):
        assert torch.isfinite(z).all() and torch.isfinite(nn).all(), f'{what}: {n} is not finite'
        assert same_bits(z, nn), f'{what}: {n} under N differs from Z, max abs diff {max_diff(z, nn):.3e}'
    g, terms = res['N']
    perturb = None
    if (row, B) in PERTURB_CASES:   # test_train.test_gradients_match_oracle's choice of the sampling
        perturb = (PERTURB, PERTURB_SEEDS) if B < 32 else PERTURB_LARGE_B
    check_gradients(gpu, kw, xy, opts, what, perturb, refs, params=P, got=(flow.param_specs, g, list(terms)))
