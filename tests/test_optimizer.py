"""The clipped, guarded Adam step (cnf_optim_step, optimizers.Adam's clipvalue / clipnorm / global_clipnorm /
use_ema / skip_nonfinite, training.ema_weights).

Float64 side: clip_np below restates the gradient transform of include/cnf.h (rules 1-4 at cnf_optim_step) and
tests/test_train.adam_np the update. The raw-ABI tests run on a table of nine tensors whose sizes sit on the slab
edges (TABLE_SIZES); the existing kernel k_adam (cnf_adam_step) is the bit-level reference of the update itself.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from arl_conditional_normalizing_flows_amd import _lib
from arl_conditional_normalizing_flows_amd._lib import check, ptr
from arl_conditional_normalizing_flows_amd.config import PRESETS
from oracle.cflow_np import OracleCFlow, synthetic_class_batch
from test_train import adam_np

EPS32 = 2.0 ** -24          # half an fp32 ulp, relative
ULP2 = 2 * 2.0 ** -23       # "2 fp32 ulp relative"
LR, B1, B2, EPSILON = (float(np.float32(x)) for x in (1e-3, 0.9, 0.999, 1e-7))   # as the C ABI passes them (fp32)


# ---------------------------------------------------------------------------------------------
# the float64 restatement of the gradient transform
# ---------------------------------------------------------------------------------------------

def clip_np(g, offsets, clipvalue=0.0, clipnorm=0.0, global_clipnorm=0.0):
    """rules 1-4: {'h' clamped gradient (fp32), 's' [T] per-tensor factors (fp32), 'gnorm' the raw global norm,
    'N' the norm rule 3 compares, 'S' (fp32), 'scales' [T] = fl32(s_t * S), 'g_eff' = fl32(h * scale_t)}"""
    assert not (clipnorm and global_clipnorm)
    g = np.asarray(g, np.float32)
    h = np.clip(g, np.float32(-clipvalue), np.float32(clipvalue)) if clipvalue else g
    T = len(offsets) - 1
    s = np.ones(T, np.float32)
    sum_h = np.zeros(T, np.float64)
    for t in range(T):
        ht = h[offsets[t]:offsets[t + 1]].astype(np.float64)
        sum_h[t] = float(np.sum(ht * ht))
        if clipnorm:
            s[t] = np.float32(clipnorm / max(math.sqrt(sum_h[t]), clipnorm))
    N = math.sqrt(float(np.sum(s.astype(np.float64) ** 2 * sum_h)))
    S = np.float32(global_clipnorm / max(N, global_clipnorm)) if global_clipnorm else np.float32(1.0)
    scales = (s * S).astype(np.float32)                       # fp32 product
    per_elem = np.repeat(scales, np.diff(np.asarray(offsets)))
    g64 = g.astype(np.float64)
    return {'h': h, 's': s, 'gnorm': math.sqrt(float(np.sum(g64 * g64))), 'N': N, 'S': S, 'scales': scales,
            'g_eff': (h * per_elem).astype(np.float32)}


HAND_OFFSETS = [0, 2, 4]
HAND_G = [3.0, 4.0, 0.6, 0.8]     # tensor norms 5 and 1


def test_clip_np_hand_worked():
    """two tensors, (3, 4) of norm 5 and (0.6, 0.8) of norm 1, worked by hand for each mode and the allowed pairs"""
    f = lambda x: np.asarray(x, np.float32)
    r = clip_np(HAND_G, HAND_OFFSETS, clipvalue=3.5)
    assert np.array_equal(r['h'], f([3, 3.5, 0.6, 0.8])) and np.array_equal(r['scales'], f([1, 1]))
    assert np.array_equal(r['g_eff'], r['h'])
    assert np.isclose(r['gnorm'], math.sqrt(26), rtol=1e-15) and np.isclose(r['N'], math.sqrt(9 + 12.25 + 1), rtol=1e-7)
    r = clip_np(HAND_G, HAND_OFFSETS, clipnorm=2.0)
    assert np.allclose(r['scales'], [0.4, 1.0], rtol=1e-7) and r['scales'][1] == 1.0
    assert np.allclose(r['g_eff'], [1.2, 1.6, 0.6, 0.8], rtol=2e-7)
    assert np.isclose(r['N'], math.sqrt(4 + 1), rtol=1e-7)            # the norm after per-tensor clipping
    r = clip_np(HAND_G, HAND_OFFSETS, global_clipnorm=2.0)
    assert np.isclose(r['N'], math.sqrt(26), rtol=1e-7)
    assert np.allclose(r['scales'], [2 / math.sqrt(26)] * 2, rtol=1e-7)
    assert np.allclose(r['g_eff'], np.array(HAND_G) * 2 / math.sqrt(26), rtol=2e-7)
    r = clip_np(HAND_G, HAND_OFFSETS, global_clipnorm=100.0)          # below the threshold: untouched
    assert np.array_equal(r['scales'], f([1, 1])) and np.array_equal(r['g_eff'], f(HAND_G))
    r = clip_np(HAND_G, HAND_OFFSETS, clipvalue=3.5, clipnorm=2.0)     # clamp first, then the norm of the clamped
    assert np.allclose(r['scales'], [2 / math.sqrt(21.25), 1.0], rtol=1e-7)
    assert np.allclose(r['g_eff'], [6 / math.sqrt(21.25), 7 / math.sqrt(21.25), 0.6, 0.8], rtol=2e-7)
    r = clip_np(HAND_G, HAND_OFFSETS, clipvalue=3.5, global_clipnorm=2.0)
    assert np.isclose(r['N'], math.sqrt(22.25), rtol=1e-7)
    assert np.allclose(r['scales'], [2 / math.sqrt(22.25)] * 2, rtol=1e-7)
    r = clip_np([0.0, 0.0, 0.6, 0.8], HAND_OFFSETS, clipnorm=0.5)      # a zero tensor: factor exactly 1, no NaN
    assert r['scales'][0] == 1.0 and np.isclose(r['scales'][1], 0.5, rtol=1e-7)


# ---------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------

def table_sizes(lib):
    s = lib.cnf_optim_slab_elems()
    return [1, 3, s - 1, s, s + 1, 2 * s + 37, 0, 1, 114688]


def table_offsets(lib):
    return [0] + [int(x) for x in np.cumsum(table_sizes(lib))]


def _c_offsets(offsets):
    return (C.c_int64 * len(offsets))(*offsets)


def build_table(lib, offsets):
    """(the table's bytes as the library builds them, number of slabs)"""
    T, n = len(offsets) - 1, offsets[-1]
    co = _c_offsets(offsets)
    nbytes = lib.cnf_optim_table_bytes(n, co, T)
    assert nbytes > 0, lib.cnf_last_error()
    host = np.zeros(nbytes, np.uint8)
    assert lib.cnf_optim_table_build(n, co, T, host.ctypes.data) == 0, lib.cnf_last_error()
    return host, int(lib.cnf_optim_num_slabs(n, co, T))


SLAB_DT = np.dtype([('start', '<i8'), ('count', '<i4'), ('tensor', '<i4')])


def test_table_matches_restatement(lib):
    s = lib.cnf_optim_slab_elems()
    assert s > 0 and s % 4 == 0
    offsets = table_offsets(lib)
    T, n = len(offsets) - 1, offsets[-1]
    exp = [(at, min(s, offsets[t + 1] - at), t) for t in range(T) for at in range(offsets[t], offsets[t + 1], s)]
    host, num_slabs = build_table(lib, offsets)
    assert num_slabs == len(exp) == sum(-(-k // s) for k in table_sizes(lib))
    tab = host[:16 * num_slabs].view(SLAB_DT)
    assert [tuple(int(x) for x in e) for e in tab] == exp
    first = host[16 * num_slabs:16 * num_slabs + 4 * (T + 1)].view('<i4')
    at = 0
    for i, (start, count, t) in enumerate(tab):
        assert start == at and 0 < count <= s                      # in order, covering [0, n) exactly once
        assert offsets[t] <= start and start + count <= offsets[t + 1]   # inside one tensor
        assert first[t] <= i < first[t + 1]
        at += count
    assert at == n
    assert first[0] == 0 and first[T] == num_slabs and np.all(np.diff(first) >= 0)
    empty = table_sizes(lib).index(0)
    assert first[empty] == first[empty + 1] and empty not in set(tab['tensor'].tolist())
    assert lib.cnf_optim_workspace_bytes(n, T, num_slabs) >= num_slabs * 20 + 4 * T


@pytest.mark.parametrize('n,offsets,T', [(0, [0, 0], 1), (4, [0, 4], 0), (4, [1, 4], 1), (4, [0, 3], 1),
                                         (4, [0, 3, 2, 4], 3), (4, None, 1)])
def test_table_rejects_bad_offsets(lib, n, offsets, T):
    """offsets that are not non-decreasing from 0 to n are refused where they are given: the table functions"""
    co = _c_offsets(offsets) if offsets is not None else None
    assert lib.cnf_optim_num_slabs(n, co, T) == -1
    assert lib.cnf_last_error().decode().startswith('cnf_optim_num_slabs: ')
    assert lib.cnf_optim_table_bytes(n, co, T) == 0
    buf = np.zeros(64, np.uint8)
    assert lib.cnf_optim_table_build(n, co, T, buf.ctypes.data) == -1
    assert lib.cnf_last_error().decode().startswith('cnf_optim_table_build: ')


def _desc(**kw):
    d = dict(lr=LR, beta_1=B1, beta_2=B2, epsilon=EPSILON, clipvalue=0.0, clipnorm=0.0, global_clipnorm=0.0,
             skip_nonfinite=0, ema_momentum=0.0)
    d.update(kw)
    return _lib.cnf_optim_desc(d['lr'], d['beta_1'], d['beta_2'], d['epsilon'], d['clipvalue'], d['clipnorm'],
                               d['global_clipnorm'], int(d['skip_nonfinite']), d['ema_momentum'])


A = 1 << 40   # a pointer that is never dereferenced
GOOD = dict(params=A, grads=A, m=A, v=A, ema=None, n=8, table=A, num_slabs=1, T=1, state=A, stats=None, scales=None,
            ws=A)
INVALID = [
    (dict(params=None), {}), (dict(grads=None), {}), (dict(m=None), {}), (dict(v=None), {}), (dict(table=None), {}),
    (dict(state=None), {}), (dict(ws=None), {}), (dict(desc=None), {}),
    (dict(n=0), {}), (dict(T=0), {}), (dict(num_slabs=0), {}),
    ({}, dict(clipvalue=-1.0)), ({}, dict(clipnorm=-1.0)), ({}, dict(global_clipnorm=-0.5)),
    ({}, dict(clipvalue=float('inf'))), ({}, dict(clipnorm=float('nan'))), ({}, dict(global_clipnorm=float('inf'))),
    ({}, dict(clipnorm=1.0, global_clipnorm=1.0)),
    ({}, dict(beta_1=1.0)), ({}, dict(beta_1=-0.1)), ({}, dict(beta_2=1.0)), ({}, dict(beta_2=float('nan'))),
    ({}, dict(epsilon=-1e-7)), ({}, dict(lr=float('inf'))), ({}, dict(lr=float('nan'))),
    ({}, dict(ema_momentum=1.0)), ({}, dict(ema_momentum=-0.1)), ({}, dict(ema_momentum=0.9)),   # the last: ema NULL
]


@pytest.mark.parametrize('args,desc', INVALID)
def test_step_rejects_before_any_launch(lib, args, desc):
    """every CNF_E_INVALID case returns before any HIP call: the pointers are never touched and no GPU is needed"""
    a = dict(GOOD)
    a.update(args)
    d = _desc(**desc)
    dref = None if 'desc' in args else C.byref(d)
    rc = lib.cnf_optim_step(a['params'], a['grads'], a['m'], a['v'], a['ema'], a['n'], a['table'], a['num_slabs'],
                            a['T'], dref, a['state'], a['stats'], a['scales'], a['ws'], None)
    assert rc == -1
    assert lib.cnf_last_error().decode().startswith('cnf_optim_step: ')


def test_adam_arguments():
    from arl_conditional_normalizing_flows_amd.optimizers import Adam
    with pytest.raises(ValueError):
        Adam(clipnorm=1, global_clipnorm=1)
    for kw in (dict(clipnorm=-1.0), dict(clipvalue=-0.5), dict(global_clipnorm=-2), dict(clipnorm=0),
               dict(clipvalue=float('nan')), dict(global_clipnorm=float('inf')),
               dict(use_ema=True, ema_momentum=1.0), dict(use_ema=True, ema_momentum=-0.1)):
        with pytest.raises(ValueError):
            Adam(**kw)
    assert not Adam(3e-4).guarded
    for kw in (dict(clipnorm=1.0), dict(clipvalue=0.5), dict(global_clipnorm=10.0), dict(use_ema=True),
               dict(skip_nonfinite=True)):
        assert Adam(3e-4, **kw).guarded, kw
    opt = Adam(3e-4, clipnorm=1.0)            # options but no tensor table: a clear error, before any launch
    p = torch.zeros(4)
    with pytest.raises(RuntimeError, match='tensor table'):
        opt.apply_flat(p, p.clone())


# ---------------------------------------------------------------------------------------------
# GPU: the raw ABI on the slab-edge table
# ---------------------------------------------------------------------------------------------

def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def same_bits(a, b):
    return np.array_equal(_bits(np.asarray(a)), _bits(np.asarray(b)))


class Rig:
    """the nine-tensor table on the device, the test vectors (shared, never modified) and one cnf_optim_step call"""

    def __init__(self, gpu):
        self.gpu = gpu
        self.lib = lib = _lib.load()
        self.offsets = table_offsets(lib)
        self.T, self.n = len(self.offsets) - 1, self.offsets[-1]
        host, self.num_slabs = build_table(lib, self.offsets)
        self.table = torch.from_numpy(host).to(gpu)
        self.ws_bytes = int(lib.cnf_optim_workspace_bytes(self.n, self.T, self.num_slabs))
        s = lib.cnf_optim_slab_elems()
        sizes = table_sizes(lib)
        rng = np.random.default_rng(5)
        g = (rng.standard_normal(self.n) * 1e-2).astype(np.float32)
        o = self.offsets
        self.t_big, self.t_small, self.t_zero, self.t_huge = 3, 2, 4, 1
        assert sizes[self.t_big] == s and sizes[self.t_small] == s - 1 and sizes[self.t_zero] == s + 1
        g[o[3]:o[4]] *= 100.0                       # norm ~ 64: far above the thresholds
        g[o[4]:o[5]] = 0.0                          # exactly zero
        g[o[1]:o[2]] = [1e20, -1e20, 1e20]          # squares overflow fp32
        self.g = g                                  # tensor 2 (norm ~ 0.64) stays below clipnorm = 1
        self.p0 = rng.standard_normal(self.n).astype(np.float32)
        self.m0 = rng.normal(0, 1e-2, self.n).astype(np.float32)
        self.v0 = (rng.standard_normal(self.n) ** 2 * 1e-4).astype(np.float32)
        self.g_finite = g.copy()                    # the same without the 1e20 tensor (EMA / end-to-end style checks)
        self.g_finite[o[1]:o[2]] = [0.5, -0.25, 0.125]
        self.ragged_last = o[6] - 1                 # last element of the 2 s + 37 tensor's ragged tail
        self.single = o[7]                          # the 1-element tensor after the empty one

    def dev(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.gpu)

    def step(self, g, p=None, m=None, v=None, ema=None, applied=0, ws_fill=None, state=None, bufs=None, **desc):
        """one call from (p0, m0, v0) (or the given host arrays) -> dict of host arrays"""
        b = bufs or self.buffers(p, m, v, ema, applied, state)
        if g is not None:
            b['g'].copy_(self.dev(g))
        if ws_fill is not None:
            b['ws'].fill_(ws_fill)
        d = _desc(**desc)
        check(self.lib.cnf_optim_step(ptr(b['p']), ptr(b['g']), ptr(b['m']), ptr(b['v']), ptr(b.get('ema')), self.n,
                                      ptr(self.table), self.num_slabs, self.T, C.byref(d), ptr(b['state']),
                                      ptr(b['stats']), ptr(b['scales']), ptr(b['ws']),
                                      torch.cuda.current_stream().cuda_stream), 'cnf_optim_step')
        return b

    def buffers(self, p=None, m=None, v=None, ema=None, applied=0, state=None):
        b = {'p': self.dev(self.p0 if p is None else p), 'm': self.dev(self.m0 if m is None else m),
             'v': self.dev(self.v0 if v is None else v), 'g': torch.empty(self.n, device=self.gpu),
             'state': torch.tensor(state if state is not None else [applied, 0], dtype=torch.int64, device=self.gpu),
             'stats': torch.full((_lib.OPTIM_STATS_FLOATS,), -7.0, device=self.gpu),
             'scales': torch.full((self.T,), -7.0, device=self.gpu),
             'ws': torch.empty(self.ws_bytes, dtype=torch.uint8, device=self.gpu)}
        if ema is not None:
            b['ema'] = self.dev(ema)
        return b

    @staticmethod
    def host(b):
        torch.cuda.synchronize()
        return {k: t.cpu().numpy() for k, t in b.items() if k not in ('ws', 'g')}

    def adam_ref(self, g_eff, step, p=None, m=None, v=None):
        """cnf_adam_step (the existing kernel) on g_eff -> host (p, m, v)"""
        p, m, v = (self.dev(a) for a in (self.p0 if p is None else p, self.m0 if m is None else m,
                                         self.v0 if v is None else v))
        check(self.lib.cnf_adam_step(ptr(p), ptr(self.dev(g_eff)), ptr(m), ptr(v), self.n, LR, B1, B2, EPSILON, step,
                                     torch.cuda.current_stream().cuda_stream), 'cnf_adam_step')
        torch.cuda.synchronize()
        return p.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy()

    def g_eff_from(self, g, scales, clipvalue):
        """g' = fl32(clamp(g) * scale) on the host, from the call's own scales"""
        h = np.clip(g, np.float32(-clipvalue), np.float32(clipvalue)) if clipvalue else g
        return (h * np.repeat(scales.astype(np.float32), np.diff(np.asarray(self.offsets)))).astype(np.float32)


@pytest.fixture(scope='module')
def rig(gpu):
    return Rig(gpu)


MODES = {'clipvalue': dict(clipvalue=0.02), 'clipnorm': dict(clipnorm=1.0), 'global': dict(global_clipnorm=1.0),
         'clipvalue+clipnorm': dict(clipvalue=0.02, clipnorm=1.0)}


def _rel(got, ref):
    return abs(float(got) - float(ref)) / abs(float(ref))


@pytest.mark.gpu
@pytest.mark.parametrize('mode', list(MODES))
def test_scales_and_stats(rig, mode):
    """scales and stats against clip_np to 2 fp32 ulp; the zero tensor's scale exactly 1; the 1e20 tensor's squares
    overflow fp32 while the fp64 sums (device and reference) stay finite"""
    kw = MODES[mode]
    ref = clip_np(rig.g, rig.offsets, **kw)
    o = rig.offsets
    with np.errstate(over='ignore'):
        assert np.isinf(np.sum(rig.g[o[1]:o[2]] * rig.g[o[1]:o[2]], dtype=np.float32))    # fp32 would overflow
    assert np.isfinite(ref['gnorm']) and np.isfinite(ref['N']) and np.all(np.isfinite(ref['scales']))
    out = rig.host(rig.step(rig.g, **kw))
    sc, st = out['scales'], out['stats']
    worst = float(np.max(np.abs(sc.astype(np.float64) - ref['scales']) / ref['scales']))
    print(f'{mode}: worst scale error {worst / 2.0 ** -23:.2f} ulp; gnorm {_rel(st[0], ref["gnorm"]) / 2.0 ** -23:.2f} '
          f'ulp, N {_rel(st[1], ref["N"]) / 2.0 ** -23:.2f} ulp')
    assert worst <= ULP2
    assert sc[rig.t_zero] == 1.0 if 'global_clipnorm' not in kw else sc[rig.t_zero] == out['stats'][5]
    assert sc[6] == sc[rig.t_zero]                       # the empty tensor: as a zero tensor
    if mode == 'clipnorm':
        assert sc[rig.t_big] < 0.05 and sc[rig.t_small] == 1.0 and sc[rig.t_huge] < 1e-19
    assert _rel(st[0], ref['gnorm']) <= ULP2 and _rel(st[1], ref['N']) <= ULP2
    assert st[2] == 0.0 and st[3] == 0.0
    assert _rel(st[5], ref['S']) <= ULP2
    assert list(out['state']) == [1, 0]


@pytest.mark.gpu
def test_zero_tensor_scale_is_exactly_one(rig):
    out = rig.host(rig.step(rig.g_finite, clipnorm=1e-3))
    assert out['scales'][rig.t_zero] == 1.0 and out['scales'][6] == 1.0
    assert np.all(np.isfinite(out['scales'])) and out['scales'][rig.t_big] < 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize('applied', [0, 1, 999])
def test_alpha_from_device_counter(rig, applied):
    out = rig.host(rig.step(rig.g_finite, applied=applied, clipnorm=1.0))
    t = applied + 1
    alpha = LR * math.sqrt(1 - B2 ** t) / (1 - B1 ** t)
    print(f'alpha at t = {t}: {_rel(out["stats"][4], alpha) / 2.0 ** -23:.2f} ulp')
    assert _rel(out['stats'][4], alpha) <= ULP2
    assert list(out['state']) == [applied + 1, 0]


def _check_update(rig, out, g_eff, step, what):
    pr, mr, vr = rig.adam_ref(g_eff, step)
    assert same_bits(out['m'], mr), f'{what}: m differs from cnf_adam_step on g\''
    assert same_bits(out['v'], vr), f'{what}: v differs from cnf_adam_step on g\''
    p64, r64, p0 = out['p'].astype(np.float64), pr.astype(np.float64), rig.p0.astype(np.float64)
    tol = 2.0 ** -23 * np.abs(r64) + 2.0 ** -22 * np.abs(r64 - p0)
    e = np.abs(p64 - r64)
    print(f'{what}: p worst error / bound {float(np.max(e / np.maximum(tol, 1e-300))):.3f}, '
          f'{int(np.sum(p64 != r64))} of {p64.size} elements differ')
    assert np.all(e <= tol), (what, int(np.argmax(e - tol)))
    assert not np.array_equal(out['p'], rig.p0)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('step', [1, 3])
def test_update_matches_existing_kernel(rig, mode, step):
    """m, v bit-equal to cnf_adam_step on g' = fl32(clamp(g) * scale) formed on the host from the call's own scales;
    p within 2^-23 |p| + 2^-22 |p - p0| (alpha may differ by an ulp between host and device)"""
    kw = MODES[mode]
    out = rig.host(rig.step(rig.g, applied=step - 1, **kw))
    g_eff = rig.g_eff_from(rig.g, out['scales'], kw.get('clipvalue', 0.0))
    _check_update(rig, out, g_eff, step, f'{mode} step {step}')


@pytest.mark.gpu
def test_skip_only_equals_plain_adam(rig):
    """every option off but skip_nonfinite, a finite gradient: m, v bit-equal to cnf_adam_step on g itself"""
    out = rig.host(rig.step(rig.g, skip_nonfinite=1))
    assert np.all(out['scales'] == 1.0)
    _check_update(rig, out, rig.g, 1, 'skip_nonfinite only')
    assert list(out['state']) == [1, 0] and out['stats'][3] == 0.0


@pytest.mark.gpu
def test_no_option_path_is_cnf_adam_step(rig):
    """Adam() through apply_flat: p, m, v bit-equal to direct cnf_adam_step calls (two steps)"""
    from arl_conditional_normalizing_flows_amd.optimizers import Adam
    opt = Adam(LR, B1, B2, EPSILON)
    assert not opt.guarded
    p = rig.dev(rig.p0)
    z = np.zeros_like(rig.p0)
    pr, mr, vr = rig.p0, z, z
    for step in (1, 2):
        opt.apply_flat(p, rig.dev(rig.g_finite))
        pr, mr, vr = rig.adam_ref(rig.g_finite, step, pr, mr, vr)
        torch.cuda.synchronize()
        assert same_bits(p.cpu().numpy(), pr) and same_bits(opt._m.cpu().numpy(), mr)
        assert same_bits(opt._v.cpu().numpy(), vr)
    assert opt.iterations == 2 and opt.steps_applied == 2 and opt.steps_skipped == 0 and opt.ema is None


@pytest.mark.gpu
@pytest.mark.parametrize('where,value', [('first', float('nan')), ('ragged_last', float('inf')),
                                         ('single', float('-inf'))])
def test_skip_nonfinite(rig, where, value):
    """an ordinary NaN / inf value in the gradient buffer: nothing is written, skipped = 1, applied = 0, the flag and
    the exact count in stats; the following finite step is step 1 (t did not advance)"""
    kw = dict(clipnorm=1.0, skip_nonfinite=1, ema_momentum=0.9)
    at = {'first': 0, 'ragged_last': rig.ragged_last, 'single': rig.single}[where]
    g = rig.g.copy()
    g[at] = value
    if where == 'first':
        g[at + 1] = float('inf')      # a second one, in the next tensor's slab: the count is exact
    n_bad = 2 if where == 'first' else 1
    e0 = (rig.p0 * np.float32(0.5)).astype(np.float32)
    b = rig.step(g, ema=e0, **kw)
    out = rig.host(b)
    for k, ref in (('p', rig.p0), ('m', rig.m0), ('v', rig.v0), ('ema', e0)):
        assert same_bits(out[k], ref), f'{k} changed in a skipped step'
    assert list(out['state']) == [0, 1]
    assert out['stats'][3] == 1.0 and out['stats'][2] == float(n_bad)
    out2 = rig.host(rig.step(rig.g, bufs=b, **kw))
    fresh = rig.host(rig.step(rig.g, ema=e0, **kw))
    assert list(out2['state']) == [1, 1] and out2['stats'][3] == 0.0 and out2['stats'][2] == 0.0
    for k in ('p', 'm', 'v', 'ema', 'scales'):
        assert same_bits(out2[k], fresh[k]), f'{k}: the step after a skip is not step 1'
    assert same_bits(out2['stats'][:2], fresh['stats'][:2]) and out2['stats'][4] == fresh['stats'][4]
    _check_update(rig, out2, rig.g_eff_from(rig.g, out2['scales'], 0.0), 1, f'after skip ({where})')


def adam_bounds(P0, G, M0, V0, step):
    """(reference p, m, v in float64, rounding bounds tol_p, tol_m, tol_v) of one k_adam step from fp32 state:
    the bound of tests/test_train.py::test_adam_step_matches_float64"""
    pr, mr, vr = adam_np(P0, G, M0, V0, step, lr=LR, b1=B1, b2=B2, eps=EPSILON)
    c1, c2 = 1 - B1, 1 - B2
    alpha = LR * math.sqrt(1 - B2 ** step) / (1 - B1 ** step)
    tol_m = EPS32 * (2 * c1 * np.abs(G - M0) + np.abs(mr))
    tol_v = EPS32 * (c2 * (G * G + 2 * np.abs(G * G - V0)) + np.abs(vr)) + 2.0 ** -126
    rv = np.sqrt(vr)
    d_sqrt = np.minimum(tol_v / (2 * np.maximum(rv, 1e-300)), np.sqrt(tol_v))
    den = rv + EPSILON
    q = alpha * np.abs(mr) / den
    tol_p = alpha * tol_m / den + q * d_sqrt / den + 6 * EPS32 * q + EPS32 * np.abs(pr)
    return pr, mr, vr, tol_p, tol_m, tol_v


@pytest.mark.gpu
def test_ema_three_steps_then_a_skip(rig):
    """Three steps (skip_nonfinite + EMA, no clipping: g' = g) against the float64 recurrence, each step taken from
    the device's own fp32 state before it, so the bound is one step's: p, m, v under k_adam's rounding bound (adam_bounds
    = test_adam_step_matches_float64's), and for e' = e + (p' - e) c, c = 1 - momentum (eps = 2^-24):
        c tol_p                       the error of p' carried through
      + eps c |p' - e|                the subtraction p' - e
      + eps c |p' - e|                c = fl32(1 - momentum) itself
      + eps (c |p' - e| + |e'|)       the product and the sum (one rounding when fused, two when not)
    Then a step with a NaN in the gradient leaves the EMA (and everything else) bit-unchanged."""
    mom = float(np.float32(0.9))
    c = 1 - mom
    kw = dict(skip_nonfinite=1, ema_momentum=mom)
    b = rig.buffers(ema=rig.p0)
    rng = np.random.default_rng(9)
    prev = rig.host(b)
    for step in (1, 2, 3):
        g = (rig.g_finite * np.float32(rng.uniform(0.5, 2.0))).astype(np.float32)
        cur = rig.host(rig.step(g, bufs=b, **kw))
        P0, G, M0, V0, E0 = (a.astype(np.float64) for a in (prev['p'], g, prev['m'], prev['v'], prev['ema']))
        pr, mr, vr, tol_p, tol_m, tol_v = adam_bounds(P0, G, M0, V0, step)
        er = E0 + (pr - E0) * c
        d = np.abs(pr - E0)
        tol_e = c * tol_p + EPS32 * (3 * c * d + np.abs(er))
        for what, ref, tol in (('m', mr, tol_m), ('v', vr, tol_v), ('p', pr, tol_p), ('ema', er, tol_e)):
            e = np.abs(cur[what].astype(np.float64) - ref)
            print(f'ema step {step} {what}: worst error / bound {float(np.max(e / np.maximum(tol, 1e-300))):.3f}')
            assert np.all(e <= tol), (step, what, int(np.argmax(e - tol)))
        assert not same_bits(cur['ema'], prev['ema'])
        prev = cur
    assert list(prev['state']) == [3, 0]
    g = rig.g_finite.copy()
    g[rig.n // 2] = float('nan')
    out = rig.host(rig.step(g, bufs=b, **kw))
    for k in ('p', 'm', 'v', 'ema'):
        assert same_bits(out[k], prev[k]), f'{k} changed in a skipped step'
    assert list(out['state']) == [3, 1]


@pytest.mark.gpu
def test_results_do_not_depend_on_workspace(rig):
    kw = dict(clipvalue=0.02, clipnorm=1.0, skip_nonfinite=1, ema_momentum=0.9)
    runs = [rig.host(rig.step(rig.g, ema=rig.p0, ws_fill=fill, **kw)) for fill in (0xFF, 0x00, 0x00)]
    for other in runs[1:]:
        for k in ('p', 'm', 'v', 'ema', 'scales', 'stats', 'state'):
            assert same_bits(runs[0][k], other[k]), k
    assert not same_bits(runs[0]['p'], rig.p0)


@pytest.mark.gpu
def test_graph_replay_advances_the_step(rig, gpu):
    """one captured cnf_optim_step (a linear chain on one stream) replayed 3 times equals 3 eager calls, counters
    included: t lives on the device"""
    kw = dict(global_clipnorm=1.0, skip_nonfinite=1, ema_momentum=0.9)
    eager = rig.buffers(ema=rig.p0)
    for _ in range(3):
        rig.step(rig.g_finite, bufs=eager, **kw)
    want = rig.host(eager)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        warm = rig.step(rig.g_finite, ema=rig.p0, **kw)   # the kernels' first launch, outside the capture
        b = rig.buffers(ema=rig.p0)
        b['g'].copy_(rig.dev(rig.g_finite))
    torch.cuda.synchronize()
    del warm
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        rig.step(None, bufs=b, **kw)
    torch.cuda.synchronize()
    assert same_bits(rig.host(b)['p'], rig.p0) and list(rig.host(b)['state']) == [0, 0]   # capture ran nothing
    with torch.cuda.stream(side):
        for _ in range(3):
            graph.replay()
    got = rig.host(b)
    assert list(got['state']) == [3, 0]
    for k in ('p', 'm', 'v', 'ema', 'scales', 'stats', 'state'):
        assert same_bits(got[k], want[k]), k


# ---------------------------------------------------------------------------------------------
# GPU: end to end through train_step
# ---------------------------------------------------------------------------------------------

def _elementwise_update_check(name_slices, p0, p1, g, exp, lr, what):
    """the element-wise rule of tests/test_train.py::test_train_step_adam_update_and_descent, with g the effective
    gradient: elements whose gradient is not near 0 within their tensor, to 1e-3 lr plus the parameter's rounding"""
    n_checked = 0
    for n, sl in name_slices:
        ga = np.abs(g[sl])
        if ga.size == 0:
            continue
        big = ga > 1e-3 * max(float(ga.max()), 1e-30)
        d = np.abs((p1[sl] - p0[sl]) - (exp[sl] - p0[sl]))
        tol = 1e-3 * lr + 2.0 ** -23 * np.abs(exp[sl])
        assert np.all(d[big] <= tol[big]), (what, n, float(np.max(d[big] / tol[big])))
        n_checked += int(big.sum())
    assert n_checked >= 0.5 * g.size, (what, n_checked, g.size)


@pytest.mark.gpu
def test_flow_train_step_global_clipnorm_and_ema_weights(gpu):
    from arl_conditional_normalizing_flows_amd import training
    from arl_conditional_normalizing_flows_amd.make_model import cFlow
    from arl_conditional_normalizing_flows_amd.optimizers import Adam
    cfg = PRESETS['tiny']
    kw = cfg.kwargs()
    flow = cFlow(**kw, device=gpu)
    flow.set_weights(OracleCFlow(**kw).init_params(7))
    H, W, D = cfg.io_shape
    xy = torch.from_numpy(synthetic_class_batch(2, H, W, cfg.x_d, seed=8)).to(gpu)
    g, _ = flow.gradients(xy)
    g = g.detach().cpu().numpy().copy()
    offsets = [o for _, o, _ in flow.param_specs] + [flow.num_params]
    gnorm = clip_np(g, offsets)['gnorm']
    c = 0.5 * gnorm
    lr = 1e-3
    opt = Adam(lr, global_clipnorm=c, use_ema=True, ema_momentum=0.5)
    flow.compile(optimizer=opt)
    p0 = flow.params.detach().cpu().numpy().astype(np.float64)
    out = flow.train_step(xy)
    assert set(out) == {'loss', 'z_loss', 'y_loss', 'detJ_loss'}
    p1 = flow.params.detach().cpu().numpy().astype(np.float64)
    ref = clip_np(g, offsets, global_clipnorm=c)
    st = opt.stats()
    assert abs(float(st['grad_norm']) - gnorm) <= ULP2 * gnorm
    assert abs(float(st['global_scale']) - 0.5) <= 1e-6 and float(st['skipped']) == 0.0
    assert opt.steps_applied == 1 and opt.steps_skipped == 0
    ge = ref['g_eff'].astype(np.float64)
    exp, _, _ = adam_np(p0, ge, np.zeros_like(ge), np.zeros_like(ge), 1, lr=lr)
    slices = [(n, slice(o, o + (int(np.prod(s)) if s else 1))) for n, o, s in flow.param_specs]
    _elementwise_update_check(slices, p0, p1, ge, exp, lr, 'flow global_clipnorm')
    # the weight average: different inside the context, the training weights back bit for bit after it
    before, _ = flow(xy, 1)
    before = before.clone()
    with training.ema_weights(flow):
        assert torch.equal(flow.params, opt.ema)
        inside, _ = flow(xy, 1)
        assert not torch.equal(inside, before)
    after, _ = flow(xy, 1)
    torch.cuda.synchronize()
    assert torch.equal(after, before)
    assert np.array_equal(flow.params.detach().cpu().numpy().astype(np.float64), p1)


@pytest.mark.gpu
def test_toy_train_step_clipnorm(gpu):
    from arl_conditional_normalizing_flows_amd import training
    from arl_conditional_normalizing_flows_amd.optimizers import Adam
    from arl_conditional_normalizing_flows_amd.toy_model import cINN_affine
    model = cINN_affine(3, 2, 6, 16, 1, device=gpu, seed=3)
    rng = np.random.default_rng(4)
    xy = torch.from_numpy(rng.standard_normal((8, 3)).astype(np.float32)).to(gpu)
    g, _ = model.gradients(xy)
    g = g.detach().cpu().numpy().copy()
    offsets = [0]
    for _, s in model.param_specs():
        offsets.append(offsets[-1] + int(np.prod(s)))
    norms = [math.sqrt(float(np.sum(g[a:b].astype(np.float64) ** 2))) for a, b in zip(offsets[:-1], offsets[1:])]
    c = float(np.median(norms))               # about half of the tensors are clipped
    lr = 1e-3
    opt = Adam(lr, clipnorm=c, use_ema=True)
    model.compile(optimizer=opt)
    p0 = model.params.detach().cpu().numpy().astype(np.float64)
    model.train_step(xy)
    p1 = model.params.detach().cpu().numpy().astype(np.float64)
    ref = clip_np(g, offsets, clipnorm=c)
    sc = opt.stats()['scales'].cpu().numpy()
    assert np.max(np.abs(sc - ref['scales']) / ref['scales']) <= ULP2
    assert 0 < int(np.sum(sc < 1.0)) < len(sc)
    ge = ref['g_eff'].astype(np.float64)
    exp, _, _ = adam_np(p0, ge, np.zeros_like(ge), np.zeros_like(ge), 1, lr=lr)
    slices = [(n, slice(a, b)) for (n, _), a, b in zip(model.param_specs(), offsets[:-1], offsets[1:])]
    _elementwise_update_check(slices, p0, p1, ge, exp, lr, 'toy clipnorm')
    before, _ = model(xy, -1)
    before = before.clone()
    with training.ema_weights(model):
        inside, _ = model(xy, -1)
        assert not torch.equal(inside, before)
    after, _ = model(xy, -1)
    assert torch.equal(after, before)
