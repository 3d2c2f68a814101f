"""The bf16x6 plane image of the streamed convs' weights ("The plane image"):
cnf_pack_params splits every k_pw / k_gc conv's fp32 weights into their three bf16 planes once per weight
update, in the byte layout the kernels keep in LDS, and the kernels stage them with a plain copy. The debug
option PRESPLIT=0 builds no such image and lets every workgroup split the fp32 image itself, as before; it
is the reference here: the plan's plane map against the fp32 image map (CPU), the packed planes against a
torch-CPU split of the parameters, and every result of the two settings bit for bit (GPU)."""
import ctypes as C
import functools

import numpy as np
import pytest

from arl_conditional_normalizing_flows_amd.config import PRESETS
from oracle.cflow_np import OracleCFlow, synthetic_class_batch, synthetic_sr_batch
from test_capi import _plan, _weight_map

DIR_WORDS = 16
(D_KIND, D_COUPLING, D_NET, D_ROLE, D_RB, D_BRANCH, D_X6, D_C, D_NR, D_W, D_NS, D_G, D_COUT, D_KROWS, D_DIL,
 D_BW) = range(DIR_WORDS)


def _kw(name):
    kw = PRESETS[name].kwargs()
    kw.pop('group_mode')
    return kw


def _unit(k, col, p, NR):
    """16-bit unit, inside a conv's plane image, of plane p of W[k][col]: plane p of K step c = k // 32 and
    column block nb = col // 16 is 1 KiB at ((c * 3 + p) * NR + nb) * 1024, in which lane (kq, i16) =
    ((k // 8) % 4, col % 16) owns 16 bytes at lane * 16 and element jj = k % 8 two of them"""
    return ((((k >> 5) * 3 + p) * NR + (col >> 4)) * 1024 + (((k >> 3) & 3) * 16 + (col & 15)) * 16 + (k & 7) * 2) // 2


def _fp32_index(d):
    """index into the fp32 kernel image of W[k][col] of directory entry d, for every (k, col) of its plane
    image (-1: outside the fp32 image: a structural zero). k_pw: the PK_1X1 / PK_TAP image [g][q][j][s],
    k = 16g + 4q + s; k_gc: the PK_Q4 image of channel quads qd = tap * cinp / 4 + ch / 4, k = tap * S + ch"""
    C_, NR, ns = int(d[D_C]), int(d[D_NR]), int(d[D_NS])
    k, col = np.meshgrid(np.arange(32 * C_), np.arange(16 * NR), indexing='ij')
    if d[D_KIND] == 0:
        qd, s, ok = k >> 2, k & 3, k < 16 * d[D_G]
    else:
        S, cinp = int(d[D_KROWS]), int(d[D_G])
        tap, ch = k // S, k % S
        qd, s, ok = tap * (cinp // 4) + ch // 4, ch % 4, (tap < 9) & (ch < cinp)
    return k, col, np.where(ok, d[D_W] + (qd * ns + col) * 4 + s, -1)


def _octet_table(d):
    """k_gc's K-octet table of directory entry d: per octet e (k = 8e .. 8e + 7, k = tap * S + ch) the band
    offsets, in bf16 elements from the pixel's tap-(0, 0) origin, of its one (S >= 8), two (S = 4) or four
    (S = 2) taps; 0 for the unused words and past the 9 taps"""
    S, dil, BW, G = int(d[D_KROWS]), int(d[D_DIL]), int(d[D_BW]), int(d[D_C])
    tapo = lambda t: ((t // 3) * dil * BW + (t % 3) * dil) * S if t < 9 else 0
    out = np.zeros((4 * G, 4), np.int64)
    for e in range(4 * G):
        if S >= 8:
            t = 8 * e // S
            out[e, 0] = tapo(t) + 8 * e - t * S if t < 9 else 0
        else:
            for j in range(8 // S):
                out[e, j] = tapo((8 // S) * e + j)
    return out.reshape(-1)


def _maps(lib, name, options):
    rc, p, keep = _plan(lib, _kw(name), options=options)
    assert rc == 0, lib.cnf_last_error()
    try:
        aux = _weight_map(lib, p, 0)
        assert aux.size == lib.cnf_plan_aux_floats(p)
        n2 = lib.cnf_plan_weight_map(p, 2, None, 0)
        x6 = np.zeros(n2, np.int64)
        if n2:
            assert lib.cnf_plan_weight_map(p, 2, x6.ctypes.data_as(C.POINTER(C.c_int64)), n2) == n2
        n3 = lib.cnf_plan_weight_map(p, 3, None, 0)
        d = np.zeros(n3, np.int64)
        if n3:
            assert lib.cnf_plan_weight_map(p, 3, d.ctypes.data_as(C.POINTER(C.c_int64)), n3) == n3
        return aux, x6, d.reshape(-1, DIR_WORDS), lib.cnf_plan_num_params(p)
    finally:
        lib.cnf_plan_destroy(p)


# tiny and small fit k_net_lds whole: NETLDS=0 streams every layer; cfg2 streams its four 32x32 layers
MAP_CASES = [('tiny', 'NETLDS=0'), ('small', 'NETLDS=0'), ('cfg2', '')]


@pytest.mark.parametrize('name,opts', MAP_CASES)
def test_plane_map_matches_the_fp32_image(lib, name, opts):
    old, x6_off, dir_off, _ = _maps(lib, name, (opts + ',PRESPLIT=0').lstrip(','))
    assert x6_off.size == 0 and dir_off.size == 0   # PRESPLIT=0: no plane region at all
    aux, x6, d, n_params = _maps(lib, name, opts or None)
    # the fp32 image is where and what it was; the plane region follows it (16-byte aligned) and has no fp32 entries
    assert np.array_equal(aux[:old.size], old)
    assert x6.size % 2 == 0 and x6.size > 0
    base = aux.size - x6.size // 2
    assert base % 4 == 0 and 0 <= base - old.size < 4
    assert np.all(aux[old.size:] == -1)
    assert len(d) > 0 and set(d[:, D_KIND]) <= {0, 1}
    pos = 0   # the images tile the region in directory order
    for e in d:
        C_, NR = int(e[D_C]), int(e[D_NR])
        assert (e[D_X6] - base) * 2 == pos and e[D_X6] % 4 == 0
        n = C_ * 3 * NR * 512
        img = x6[pos:pos + n]
        k, col, src = _fp32_index(e)
        par = np.where(src >= 0, old[np.maximum(src, 0)], -1)
        exp = -np.ones(n, np.int64)
        seen = np.zeros(n, np.int64)
        for p in range(3):
            u = _unit(k, col, p, NR)
            np.add.at(seen, u.reshape(-1), 1)
            exp[u] = np.where(par >= 0, 4 * par + p, -1)
        assert np.all(seen == 1)   # every slot of the image is one (k, col, plane)
        assert np.array_equal(img, exp), tuple(e)
        # nothing of the conv is left out: the image's parameters are the fp32 image's
        size = (16 * int(e[D_G]) if e[D_KIND] == 0 else (9 * int(e[D_G]) // 4 + 3) // 4 * 16) * int(e[D_NS])
        fp = old[e[D_W]:e[D_W] + size]
        assert np.array_equal(np.unique(par[par >= 0]), np.unique(fp[fp >= 0]))
        assert np.all(img[img >= 0] >> 2 < n_params)
        pos += n
        if e[D_KIND] == 1:   # the K-octet table: ints as two literal 16-bit halves, low first
            t = -2 - x6[pos:pos + 32 * C_]
            assert np.all((t >= 0) & (t < 65536))
            assert np.array_equal(t[0::2] | (t[1::2] << 16), _octet_table(e))
            pos += 32 * C_
    assert pos == x6.size
    if name == 'cfg2':   # conv_in, conv_a, conv_b and conv_out of k_pw; k_gc branches of S = 8, 4, 2
        assert set(d[d[:, D_KIND] == 0][:, D_ROLE]) == {0, 1, 3, 4}
        assert set(d[d[:, D_KIND] == 1][:, D_KROWS]) == {8, 4, 2}


def test_presplit_option_is_parsed(lib):
    kw = _kw('small')
    for bad in ('PRESPLIT=2', 'PRESPLIT=-1', 'PRESPLIT', 'PRESPLIT=x'):
        rc, p, keep = _plan(lib, kw, options=bad)
        assert rc == -1 and not p.value, bad
        assert b'debug_options' in lib.cnf_last_error()
    sizes = []
    for good in ('NETLDS=0,PRESPLIT=0', 'NETLDS=0,PRESPLIT=1', 'NETLDS=0'):
        rc, p, keep = _plan(lib, kw, options=good)
        assert rc == 0, good
        sizes.append(lib.cnf_plan_aux_floats(p))
        lib.cnf_plan_destroy(p)
    assert sizes[0] < sizes[1] == sizes[2]   # the default is PRESPLIT=1


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _params(name, seed=0):
    return OracleCFlow(**PRESETS[name].kwargs()).init_params(seed)


@functools.lru_cache(maxsize=None)
def _batch(name, B):
    cfg = PRESETS[name]
    H, W, D = cfg.io_shape
    if cfg.data == 'class':
        return synthetic_class_batch(B, H, W, cfg.x_d, seed=1)
    return synthetic_sr_batch(B, H, W, cfg.x_d, cfg.sr_pow, seed=1)


def _flow(name, gpu, options, seed=0):
    from arl_conditional_normalizing_flows_amd.make_model import cFlow
    flow = cFlow(**PRESETS[name].kwargs(), device=gpu, debug_options=options or None)
    flow.set_weights(_params(name, seed))
    return flow


def _results(flow, x):
    zy, ld = flow(x, 1, per_image_logdet=True)
    return zy.clone(), ld.clone(), flow(zy, -1).clone()


def _split(x):
    """the issue's reference split on the CPU: h = bf16(x), m = bf16(x - h), l = bf16(x - h - m)"""
    import torch
    h = x.bfloat16()
    m = (x - h).bfloat16()
    l = (x - h - m).bfloat16()
    return [t.view(torch.int16).numpy().view(np.uint16) for t in (h, m, l)]


@pytest.mark.gpu
def test_packed_planes_are_the_cpu_split(gpu, lib):
    """cfg2 after cnf_pack_params: the whole plane region equals the torch-CPU split of the parameters its map
    names, bit for bit; and, without the map, one k_pw conv (conv_b) and one k_gc branch of each of S = 8, 4, 2
    hold at the documented address of every (k, column, plane) the split of that element of the fp32 image."""
    import torch
    flow = _flow('cfg2', gpu, None)
    torch.cuda.synchronize()
    aux, x6, d, _ = _maps(lib, 'cfg2', None)
    base = aux.size - x6.size // 2
    dev_aux = flow._aux.cpu()
    assert dev_aux.numel() == aux.size
    got = dev_aux[base:].view(torch.int16).numpy().view(np.uint16)
    planes = _split(flow.params.cpu())
    exp = np.zeros(x6.size, np.uint16)
    for p in range(3):
        m = (x6 >= 0) & ((x6 & 3) == p)
        exp[m] = planes[p][x6[m] >> 2]
    lit = x6 <= -2
    exp[lit] = (-2 - x6[lit]).astype(np.uint16)
    assert np.array_equal(got, exp)
    assert np.count_nonzero(got) > x6.size // 4
    # the documented layout, from the fp32 image's own values
    picks = [d[(d[:, D_KIND] == 0) & (d[:, D_ROLE] == 3)][0]]
    picks += [d[(d[:, D_KIND] == 1) & (d[:, D_KROWS] == S)][0] for S in (8, 4, 2)]
    fp32 = dev_aux[:base]
    for e in picks:
        k, col, src = _fp32_index(e)
        w = torch.where(torch.from_numpy(src >= 0), fp32[torch.from_numpy(np.maximum(src, 0))], torch.zeros(()))
        img = got[(e[D_X6] - base) * 2:]
        for p, pl in enumerate(_split(w)):
            assert np.array_equal(img[_unit(k, col, p, int(e[D_NR]))], pl), (tuple(e), p)


RESULT_CASES = [('cfg2', 5, ''), ('cfg2', 5, 'GENERIC=6'), ('small', 3, 'NETLDS=0'), ('tiny', 2, 'NETLDS=0'),
                ('narrow', 2, 'NETLDS=0'), ('cfg4', 2, ''), ('cfg5', 1, '')]


@pytest.mark.gpu
@pytest.mark.parametrize('name,B,opts', RESULT_CASES)
def test_results_equal_presplit_off(gpu, name, B, opts):
    """zy, the per-image log-det and the inverse with the plane image against PRESPLIT=0, bit for bit"""
    import torch
    x = torch.from_numpy(_batch(name, B)).to(gpu)
    new = _results(_flow(name, gpu, opts), x)
    old = _results(_flow(name, gpu, (opts + ',PRESPLIT=0').lstrip(',')), x)
    for a, b, what in zip(new, old, ('zy', 'logdet', 'inverse')):
        assert torch.equal(a, b), what
    assert torch.isfinite(new[0]).all() and new[0].abs().max() > 0


@pytest.mark.gpu
def test_planes_follow_the_weights(gpu):
    """set_weights and train_step repack the planes: after either, the forward with the plane image equals the
    PRESPLIT=0 forward on the same weights, and differs from the forward before the update"""
    import torch
    x = torch.from_numpy(_batch('small', 3)).to(gpu)
    f1, f0 = _flow('small', gpu, 'NETLDS=0'), _flow('small', gpu, 'NETLDS=0,PRESPLIT=0')
    before = _results(f1, x)
    for f in (f1, f0):
        f.set_weights(_params('small', 1))
    after = _results(f1, x)
    for a, b in zip(after, _results(f0, x)):
        assert torch.equal(a, b)
    assert not torch.equal(after[0], before[0])
    f1.train_step(x)
    f0.set_weights(f1.params.clone())
    stepped = _results(f1, x)
    for a, b in zip(stepped, _results(f0, x)):
        assert torch.equal(a, b)
    assert not torch.equal(stepped[0], after[0])


@pytest.mark.gpu
def test_training_forward_gradients_equal(gpu):
    """one cFlow.gradients call on small with every layer streamed (the training forward's dual-store conv_a
    among its k_pw launches): gradients and loss terms bit for bit between the two settings"""
    import torch
    x = torch.from_numpy(_batch('small', 3)).to(gpu)
    g1, t1 = _flow('small', gpu, 'NETLDS=0').gradients(x)
    g1, t1 = g1.clone(), [v.clone() for v in t1]
    g0, t0 = _flow('small', gpu, 'NETLDS=0,PRESPLIT=0').gradients(x)
    assert torch.equal(g1, g0) and g1.abs().max() > 0
    for a, b in zip(t1, t0):
        assert torch.equal(a, b)
