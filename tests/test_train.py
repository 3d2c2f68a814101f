"""NLL training step (cFlow.train_step, conv_cINN_make_model.py:1850-1880).

Gradient oracle: torch autograd (float64) over oracle.cflow_torch_cpu.TorchCPUFlow, the op-for-op
restatement of the reference graph (its forward is pinned to the numpy oracle in
tests/test_oracle.py). The autograd conventions that matter are TF's: d|x|/dx = sign(x) (0 at 0),
LeakyReLU'(x) = 1 if x > 0 else alpha, LayerNorm with biased variance. CPU tests check the oracle's
gradient against central finite differences and the Keras Adam restatement; the GPU tests compare
the HIP backward (cnf_flow_backward through the C ABI) per parameter tensor.

Tolerance. The loss is piecewise smooth: LeakyReLU (and |y - y'|) have kinks, and the deep
configurations put millions of activations through them, some within 1e-7 of a kink. An fp32
forward differs from float64 by ~1e-6 relative, so a few activations sit on the other side of a
kink and the gradient of whole tensors moves by a DISCRETE amount (cfg2 B=2: float64 autograd
itself moves by 7.5e-3 relative in layer c11, 2e-1 in c5, when xy is perturbed by 1e-7..1e-6
relative, while each layer's own VJP at the float64 activations matches to ~1e-6). The bar is
therefore, per parameter tensor, with g_ref the float64 gradient, g32 torch fp32 autograd and
spread = max over 9 float64 gradients at xy * (1 + eps * N(0,1)), eps in PERTURB, of |g_pert - g_ref|:
  max|g - g_ref| <= K * max|g32 - g_ref| + KP * max(spread)
                    + GRAD_RTOL * max|g_ref| + GRAD_ATOL * max_all|g_ref|,
K = K32_LAYER for one coupling layer's backward (no perturbation term: the strict per-layer bar of
test_coupling_layer_vjp_matches_oracle), K32 for the whole flow."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from arl_conditional_normalizing_flows_amd.config import PRESETS
from oracle.cflow_np import OracleCFlow, synthetic_class_batch, synthetic_sr_batch
from oracle.cflow_torch_cpu import TorchCPUFlow

K32 = 10.0        # whole flow: 16 layers of fp32 rounding compound differently than torch's
K32_LAYER = 4.0   # one coupling layer
# relative input perturbations ~ the fp32 forward's own rounding, which compounds over the 16
# layers: by c7 the HIP forward's activations sit a few 1e-6 from the float64 ones
PERTURB = (1e-7, 1e-6, 4e-6)
PERTURB_SEEDS = 3         # seeds per eps: the spread is a sampled estimate
PERTURB_CASES = ('cfg2',)  # deep enough for kink flips (the small presets pass without the term)
KP = 2.0          # whole flow: multiple of the float64 gradient's spread under PERTURB
GRAD_RTOL = 1e-4
GRAD_ATOL = 1e-5


def _batch(cfg, B, seed):
    H, W, D = cfg.io_shape
    if cfg.data == 'class':
        return synthetic_class_batch(B, H, W, cfg.x_d, seed=seed)
    return synthetic_sr_batch(B, H, W, cfg.x_d, cfg.sr_pow, seed=seed)


def oracle_grads(kw, P, xy, dtype=torch.float64):
    """autograd gradient of the reference loss; returns ({name: float64 grad}, loss terms)."""
    tf = TorchCPUFlow(**kw)
    T = {k: torch.tensor(np.asarray(v, np.float64), dtype=dtype, requires_grad=True) for k, v in P.items()}
    terms = tf.log_loss(torch.from_numpy(np.asarray(xy, np.float64)).to(dtype), T)
    terms[0].backward()
    return {k: v.grad.double().numpy().copy() for k, v in T.items()}, [float(t.detach()) for t in terms]


def _tol(ref, g32, gmax, k=K32):
    return k * float(np.max(np.abs(g32 - ref))) + GRAD_RTOL * float(np.max(np.abs(ref))) + GRAD_ATOL * gmax


def adam_np(p, g, m, v, t, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7):
    """keras Adam restatement (float64)."""
    m = m + (g - m) * (1 - b1)
    v = v + (g * g - v) * (1 - b2)
    alpha = lr * math.sqrt(1 - b2 ** t) / (1 - b1 ** t)
    return p - alpha * m / (np.sqrt(v) + eps), m, v


# ---------------------------------------------------------------------------------------------
# CPU: the oracle itself
# ---------------------------------------------------------------------------------------------

def test_oracle_gradient_matches_finite_differences():
    cfg = PRESETS['tiny']
    kw = cfg.kwargs()
    ora = OracleCFlow(**kw)
    P = ora.init_params(3)
    xy = _batch(cfg, 2, 4)
    G, _ = oracle_grads(kw, P, xy)
    tf = TorchCPUFlow(**kw)
    rng = np.random.default_rng(0)

    def loss(Pd):
        T = {k: torch.tensor(np.asarray(v, np.float64)) for k, v in Pd.items()}
        return float(tf.log_loss(torch.from_numpy(np.asarray(xy, np.float64)), T)[0])

    names = sorted(P)
    checked = 0
    for name in rng.choice(names, size=8, replace=False):
        a = np.asarray(P[name], np.float64)
        idx = tuple(int(rng.integers(0, s)) for s in a.shape) if a.shape else ()
        eps = 1e-6
        Pp = dict(P)
        Pm = dict(P)
        ap, am = a.copy(), a.copy()
        ap[idx] += eps
        am[idx] -= eps
        Pp[name], Pm[name] = ap, am
        fd = (loss(Pp) - loss(Pm)) / (2 * eps)
        g = G[name][idx]
        assert abs(fd - g) <= 1e-4 * max(1.0, abs(g)), (name, idx, fd, g)   # |y - y'| kinks bound the FD accuracy
        checked += 1
    assert checked == 8


def test_adam_restatement_first_step():
    # step 1: m = 0.1 g, v = 0.001 g^2, alpha = lr sqrt(0.001)/0.1 -> update ~ lr * sign(g)
    g = np.array([0.5, -2.0, 1e-2])
    p, m, v = adam_np(np.zeros(3), g, np.zeros(3), np.zeros(3), 1, lr=1e-2)
    assert np.allclose(p, -1e-2 * np.sign(g), rtol=1e-3)


def test_train_workspace_is_larger_than_inference(lib):
    from arl_conditional_normalizing_flows_amd import _lib
    cfg = PRESETS['small']
    kw = cfg.kwargs()
    lists = [(C.c_int * len(kw[k]))(*kw[k]) for k in ('squeeze_factor_block_list', 'ResNeXt_block_list',
                                                        'num_kernels_list', 'cardinality_list')]
    d = _lib.cnf_flow_desc(*kw['io_shape'], kw['x_d'], len(lists[0]), *lists, 100.0, 3, 1, 1, 0)
    plan = C.c_void_p()
    assert lib.cnf_plan_create(C.byref(d), C.byref(plan)) == 0
    try:
        inf = lib.cnf_plan_workspace_bytes(plan, 4)
        tr = lib.cnf_plan_train_workspace_bytes(plan, 4)
        assert tr > inf > 0
    finally:
        lib.cnf_plan_destroy(plan)


# ---------------------------------------------------------------------------------------------
# GPU: the HIP backward and the training step
# ---------------------------------------------------------------------------------------------

def _gpu_flow(kw, P, gpu, options=None):
    from arl_conditional_normalizing_flows_amd.make_model import cFlow
    flow = cFlow(**kw, device=gpu, debug_options=options)
    flow.set_weights(P)
    return flow


GRAD_CASES = [('tiny', 2, {}), ('small', 3, {}), ('small', 2, {'group_mode': 'intended'}),
              ('tiny', 2, {'LAYER_NORM': False}), ('cfg2', 2, {}),
              # no LayerNorm on streamed (not LDS-resident) layers: conv_a's saved t1 by its own launch
              ('cfg2', 2, {'LAYER_NORM': False}),
              # couplings 2 and 1 pixels wide: the weight gradients fall back to the VALU k_wgrad
              ('narrow', 3, {}),
              # every training convolution on the VALU kernels (k_tconv, k_wgrad; debug option TRAIN_ALT bit 1)
              ('small', 3, {'_opts': {'TRAIN_ALT': 1}}),
              # the multi-kernel backward for the k_net_lds layers too (LDS_BWD=0; by default they run the
              # fused k_lds_bwd over the training forward's saved activations)
              ('small', 3, {'_opts': {'LDS_BWD': 0}}), ('cfg2', 2, {'_opts': {'LDS_BWD': 0}}),
              # the LDS-staged band weight gradients (k_wgrad_band) instead of the register-operand
              # k_wgrad_direct (TRAIN_ALT bit 2), and the MFMA kernels for the thin-channel ones (bit 8)
              ('cfg2', 2, {'_opts': {'TRAIN_ALT': 2}}), ('cfg2', 2, {'_opts': {'TRAIN_ALT': 8}}),
              # the LDS layers' backward as one launch per layer (LDS_BWD=1) instead of the data-gradient
              # chain and the weight gradients as two launches on two streams
              ('cfg2', 2, {'_opts': {'LDS_BWD': 1}}), ('small', 3, {'_opts': {'LDS_BWD': 1}}),
              # the streamed layers' LN-backward reduction as its own kernel (k_lnb_reduce) instead of fused
              # into the producing data-gradient kernel (TRAIN_ALT bit 16)
              ('cfg2', 2, {'_opts': {'TRAIN_ALT': 16}}),
              # dt1's gradient buffer zeroed before the grouped branches (TRAIN_ALT bit 32) instead of the LN2
              # backward masking the channels outside the branch windows
              ('cfg2', 2, {'_opts': {'TRAIN_ALT': 32}}),
              # the streamed layers' activations recomputed in the backward instead of saved (TRAIN_SCHED bit 2)
              # and net A's chain enqueued before net b's (bit 4)
              ('cfg2', 2, {'_opts': {'TRAIN_SCHED': 6}}),
              # the benched training batch (bench.py --mode train): the batch-sliced LN backward (up to 8
              # workgroups per image), the multi-unit band weight gradients and the four-stream schedule
              # all see their full-size partitions only here
              ('cfg2', 64, {})]
# at the bench batch the float64 spread is sampled more sparsely (each float64 autograd pass of
# cfg2 B=64 takes ~20 s on the box's 16 host threads)
PERTURB_LARGE_B = ((1e-6, 4e-6), 1)


@pytest.mark.gpu
@pytest.mark.parametrize('name,B,extra', GRAD_CASES)
def test_gradients_match_oracle(gpu, name, B, extra):
    extra = dict(extra)
    options = extra.pop('_opts', None)
    cfg = PRESETS[name]
    kw = dict(cfg.kwargs(), **extra)
    xy = _batch(cfg, B, 6)
    perturb = None
    if name in PERTURB_CASES:
        perturb = (PERTURB, PERTURB_SEEDS) if B < 32 else PERTURB_LARGE_B
    check_gradients(gpu, kw, xy, options, f'{name} {extra}', perturb)


def check_gradients(gpu, kw, xy, options=None, label='', perturb=None, refs=None, params=None, got=None):
    """The HIP gradient of the flow cFlow(**kw) at xy (weights params, by default init_params(5)) and its 4
    loss terms against float64 autograd, under the module docstring's bar. perturb: None (no perturbation
    term) or (eps list, seeds per eps). refs: (G_ref, terms_ref, G32) of this kw, xy and params when the
    caller has them already. got: (param_specs, gradient, loss terms) of a flow.gradients(xy) call the
    caller made on such a flow (then none is made here)."""
    B = xy.shape[0]
    ora = OracleCFlow(**kw)
    P = ora.init_params(5) if params is None else params
    if refs is None:
        G_ref, terms_ref = oracle_grads(kw, P, xy)
        G32, _ = oracle_grads(kw, P, xy, torch.float32)
    else:
        G_ref, terms_ref, G32 = refs
    # float64 gradient's own spread under input perturbations of the fp32 forward's rounding size
    G_spread = {k: np.zeros(np.size(v)) for k, v in G_ref.items()}
    if perturb is not None:
        rng = np.random.default_rng(11)
        eps_list, seeds = perturb
        for eps in eps_list:
            for _ in range(seeds):
                Gp, _ = oracle_grads(kw, P, np.asarray(xy, np.float64) * (1.0 + eps * rng.standard_normal(xy.shape)))
                for k in G_spread:
                    G_spread[k] = np.maximum(G_spread[k], np.abs(Gp[k].reshape(-1) - G_ref[k].reshape(-1)))
    if got is None:
        flow = _gpu_flow(kw, P, gpu, options)
        g, terms = flow.gradients(torch.from_numpy(xy).to(gpu))
        param_specs = flow.param_specs
    else:
        param_specs, g, terms = got
    g = g.cpu().numpy().astype(np.float64)
    terms = [float(t) for t in terms]
    # the north-star bound of the forward parity tests (test_gpu_parity.test_nll_matches_oracle): 1e-5 of
    # max(|ref|, mean over images of sum|s|) -- the log-det terms' conditioning scale
    _, _, abs_s = ora.forward(np.asarray(xy, np.float64), P, abs_s=True)
    # (round 4 used 1e-4 * max(1, |r|); both bounds are printed so that a term the new one admits and the
    # old one would not is visible)
    for r, t in zip(terms_ref, terms):
        bound = 1e-5 * max(abs(r), float(np.mean(abs_s)))
        print(f'loss term {r:.6e}: |err| {abs(r - t):.2e}, bound {bound:.2e} (round-4 bound {1e-4 * max(1.0, abs(r)):.2e})')
        assert abs(r - t) <= bound, (terms_ref, terms)
    gmax = max(float(np.max(np.abs(v))) for v in G_ref.values())
    worst = (0.0, '')
    bad = []
    for n, o, s in param_specs:
        size = int(np.prod(s)) if s else 1
        ref = np.asarray(G_ref[n], np.float64).reshape(-1)
        got = g[o:o + size]
        g32 = np.asarray(G32[n]).reshape(-1)
        err = float(np.max(np.abs(got - ref)))
        tol = _tol(ref, g32, gmax) + KP * float(np.max(G_spread[n]))
        worst = max(worst, (err / max(tol, 1e-30), n))
        if err > tol:
            bad.append(f'{n}: max|dg| {err:.3e} > tol {tol:.3e} (max|g_ref| {np.max(np.abs(ref)):.3e}, '
                       f'fp32 autograd err {np.max(np.abs(g32 - ref)):.3e})')
    print(f'{label} B={B}: worst gradient error / tolerance {worst[0]:.3f} ({worst[1]}), max|g| {gmax:.3e}')
    assert not bad, '\n'.join(bad)


@pytest.mark.gpu
def test_gradients_bitwise_reproducible_across_runs_and_streams(gpu):
    """The training backward at the benched batch (cfg2 B=64) is atomic-free and every multi-stream
    join is event-ordered with the u1 gradients added in a fixed order: two runs give the same
    gradient bit for bit, and so does the single-stream schedule of the weight gradients
    (debug option TRAIN_SCHED bit 1) — a missing event or a wrong slice count would show here."""
    cfg = PRESETS['cfg2']
    kw = cfg.kwargs()
    P = OracleCFlow(**kw).init_params(5)
    xy = torch.from_numpy(_batch(cfg, 64, 6)).to(gpu)
    flow = _gpu_flow(kw, P, gpu)
    g1 = flow.gradients(xy)[0].clone()
    g2 = flow.gradients(xy)[0].clone()
    g3 = _gpu_flow(kw, P, gpu, {'TRAIN_SCHED': 1}).gradients(xy)[0].clone()
    torch.cuda.synchronize()
    assert torch.isfinite(g1).all()
    assert torch.equal(g1, g2)
    assert torch.equal(g1, g3)


@pytest.mark.gpu
def test_train_step_adam_update_and_descent(gpu):
    from arl_conditional_normalizing_flows_amd.optimizers import Adam
    cfg = PRESETS['small']
    kw = cfg.kwargs()
    ora = OracleCFlow(**kw)
    P = ora.init_params(7)
    xy = torch.from_numpy(_batch(cfg, 4, 8)).to(gpu)
    flow = _gpu_flow(kw, P, gpu)
    flow.compile(optimizer=Adam(learning_rate=1e-5))
    p0 = flow.params.detach().cpu().numpy().astype(np.float64)
    g, _ = flow.gradients(xy)
    g = g.detach().cpu().numpy().astype(np.float64)
    out = flow.train_step(xy)
    assert set(out) == {'loss', 'z_loss', 'y_loss', 'detJ_loss'}
    p1 = flow.params.detach().cpu().numpy().astype(np.float64)
    lr = 1e-5
    exp, _, _ = adam_np(p0, g, np.zeros_like(g), np.zeros_like(g), 1, lr=lr)
    assert np.max(np.abs(p1 - exp)) <= 1e-6 + 1e-5 * np.max(np.abs(exp))
    # the bound above is wider than the update itself (|update| <= lr, the bound ~ 1e-5 max|p|). The update:
    # on the elements whose gradient is not near 0 within its tensor, to 1e-3 lr plus the fp32 rounding of
    # the parameter (the rule of test_training_driver.test_fit_trajectory_matches_float64_oracle)
    n_checked = 0
    for n, o, s in flow.param_specs:
        sl = slice(o, o + (int(np.prod(s)) if s else 1))
        ga = np.abs(g[sl])
        big = ga > 1e-3 * max(float(ga.max()), 1e-30)
        d = np.abs((p1[sl] - p0[sl]) - (exp[sl] - p0[sl]))
        tol = 1e-3 * lr + 2.0 ** -23 * np.abs(exp[sl])
        assert np.all(d[big] <= tol[big]), (n, float(np.max(d[big] / tol[big])))
        n_checked += int(big.sum())
    assert n_checked >= 0.5 * g.size, (n_checked, g.size)
    # a few more steps on the same batch lower the loss
    losses = [out['loss']]
    for _ in range(5):
        flow.loss_tracker.reset_state()
        losses.append(flow.train_step(xy)['loss'])
    print('train_step losses', losses)
    assert losses[-1] < losses[0]
    # forward / inverse still consistent after the update (aux image repacked)
    zy, _ = flow(xy, 1)
    x2 = flow(zy, -1)
    assert float((x2 - xy).abs().max()) <= 1e-4 * float(xy.abs().max())


@pytest.mark.gpu
def test_adam_step_matches_float64(gpu):
    """cnf_adam_step (k_adam) alone against adam_np in float64: n = 8192 * 256 + 37, so the grid-stride
    loop (the launch is capped at 8192 workgroups of 256) and a ragged tail both run; non-zero m and v
    (and a zero block); steps 1, 2 and 1000; gradients over seven decades with 0, +-1e-20 (g^2 underflows:
    epsilon decides) and +-1e3 placed at the start and in the tail. p, m and v to the fp32 rounding of the
    float64 result, each bound the sum of the roundings of the kernel's own operations (eps = 2^-24):
      m' = m + (g - m) c1            : eps (2 c1 |g - m| + |m'|)
      v' = v + (g g - v) c2          : eps (c2 (g^2 + 2 |g^2 - v|) + |v'|), plus the smallest normal (g^2 may flush)
      p' = p - alpha m' / (sqrt(v') + epsilon): the above carried through (|sqrt a - sqrt b| <= min(|a - b| /
           (2 sqrt b), sqrt|a - b|)), 6 eps of the quotient for sqrt, the sum, alpha, the product and the
           division, and eps |p'|.
    The reference takes lr, beta and epsilon as the fp32 values the C ABI passes."""
    from arl_conditional_normalizing_flows_amd import _lib
    from arl_conditional_normalizing_flows_amd._lib import check, ptr
    lib = _lib.load()
    n = 8192 * 256 + 37
    rng = np.random.default_rng(21)
    p0 = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 1, n)).astype(np.float32)
    m0 = rng.normal(0, 0.1, n).astype(np.float32)
    v0 = (rng.standard_normal(n) ** 2 * 1e-2).astype(np.float32)
    special = np.array([0.0, 1e-20, -1e-20, 1e3, -1e3], np.float32)
    for at in (0, 8192 * 256 + 20):              # first workgroup, and the ragged tail
        g[at:at + 5] = special
    for at in (5, 8192 * 256 + 25):              # the same gradients on zero moments
        g[at:at + 5] = special
        m0[at:at + 5] = 0
        v0[at:at + 5] = 0
    m0[1000:2000] = 0
    v0[1000:2000] = 0
    lr, b1, b2, epsilon = (float(np.float32(x)) for x in (1e-3, 0.9, 0.999, 1e-7))
    eps = 2.0 ** -24
    for step in (1, 2, 1000):
        p, m, v = (torch.from_numpy(a.copy()).to(gpu) for a in (p0, m0, v0))
        check(lib.cnf_adam_step(ptr(p), ptr(torch.from_numpy(g).to(gpu)), ptr(m), ptr(v), n, lr, b1, b2, epsilon, step,
                                torch.cuda.current_stream().cuda_stream), 'cnf_adam_step')
        torch.cuda.synchronize()
        P0, G, M0, V0 = (a.astype(np.float64) for a in (p0, g, m0, v0))
        pr, mr, vr = adam_np(P0, G, M0, V0, step, lr=lr, b1=b1, b2=b2, eps=epsilon)
        c1, c2 = 1 - b1, 1 - b2
        alpha = lr * math.sqrt(1 - b2 ** step) / (1 - b1 ** step)
        tol_m = eps * (2 * c1 * np.abs(G - M0) + np.abs(mr))
        tol_v = eps * (c2 * (G * G + 2 * np.abs(G * G - V0)) + np.abs(vr)) + 2.0 ** -126
        rv = np.sqrt(vr)
        d_sqrt = np.minimum(tol_v / (2 * np.maximum(rv, 1e-300)), np.sqrt(tol_v))
        den = rv + epsilon
        q = alpha * np.abs(mr) / den
        tol_p = alpha * tol_m / den + q * d_sqrt / den + 6 * eps * q + eps * np.abs(pr)
        for what, got, ref, tol in (('m', m, mr, tol_m), ('v', v, vr, tol_v), ('p', p, pr, tol_p)):
            e = np.abs(got.cpu().numpy().astype(np.float64) - ref)
            print(f'adam step {step} {what}: worst error / bound {np.max(e / np.maximum(tol, 1e-300)):.3f}')
            assert np.all(e <= tol), (step, what, int(np.argmax(e / tol)), float(np.max(e / np.maximum(tol, 1e-300))))
        assert not np.array_equal(p.cpu().numpy()[-37:], p0[-37:])   # the tail was updated


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['small', 'cfg2'])
def test_coupling_layer_vjp_matches_oracle(gpu, name):
    """Per-layer backward (cnf_coupling_backward) for every coupling layer: random u, dv and
    dlogdet against torch float64 autograd of the oracle coupling (TorchCPUFlow._coupling)."""
    cfg = PRESETS[name]
    kw = cfg.kwargs()
    ora = OracleCFlow(**kw)
    P = ora.init_params(9)
    flow = _gpu_flow(kw, P, gpu)
    tf = TorchCPUFlow(**kw)
    couplings = [e.coupling for e in tf.layers if e.kind == 'coupling']
    layers = [L for L in flow.layers_list if hasattr(L, 'coupling_index')]
    rng = np.random.default_rng(1)
    B, g_ld = 2, -0.37
    worst = []
    for L, c in zip(layers, couplings):
        shp = (B, L.input_height, L.input_width, L.input_depth)
        u = rng.standard_normal(shp)
        dv = rng.standard_normal(shp)
        grads = {}
        for dt in (torch.float64, torch.float32):
            T = {k: torch.tensor(np.asarray(v, np.float64), dtype=dt, requires_grad=True) for k, v in P.items()
                 if k.startswith(f'c{c.index}.')}
            ut = torch.tensor(u, dtype=dt, requires_grad=True)
            v, ld = tf._coupling(ut, c, T, +1)
            (torch.sum(v * torch.from_numpy(dv).to(dt)) + g_ld * B * ld).backward()
            grads[dt] = ({k: t.grad.double().numpy().reshape(-1) for k, t in T.items()}, ut.grad.double().numpy())
        (G, gu), (G32, gu32) = grads[torch.float64], grads[torch.float32]
        du, dp = L.gradients(torch.from_numpy(u).float().to(gpu), torch.from_numpy(dv).float().to(gpu), g_ld)
        du = du.cpu().numpy()
        dp = dp.cpu().numpy().astype(np.float64)
        e_u = float(np.max(np.abs(du - gu)))
        tol_u = _tol(gu, gu32, 0.0, K32_LAYER)
        gmax = max(float(np.max(np.abs(v))) for v in G.values())
        rel = 0.0
        for n, o, s in flow.param_specs:
            if n not in G:
                continue
            size = int(np.prod(s)) if s else 1
            err = float(np.max(np.abs(dp[o:o + size] - G[n])))
            tol = _tol(G[n], G32[n], gmax, K32_LAYER)
            rel = max(rel, err / tol)
            assert err <= tol, (c.index, n, err, tol, float(np.max(np.abs(G[n]))))
        worst.append((c.index, e_u / tol_u, rel))
        assert e_u <= tol_u, (c.index, e_u, tol_u)
    print(name, ' '.join(f'c{i}: du/tol {a:.2f} dp/tol {b:.2f}' for i, a, b in worst))


@pytest.mark.gpu
def test_flow_layer_vjps_at_oracle_activations(gpu):
    """Every coupling layer's HIP backward at the TRUE activations of a cfg2 flow: u = the float64
    forward's input to the layer, dv = the float64 gradient of the reference loss at its output,
    per-image log-det cotangent -1/B (loss = -(mean ll + mean log-det)). Isolates the backward
    kernels from the kink flips of the whole-flow comparison (module docstring): strict per-layer
    bar against float64 and torch fp32 autograd of the same layer."""
    cfg = PRESETS['cfg2']
    kw = cfg.kwargs()
    ora = OracleCFlow(**kw)
    P = ora.init_params(5)
    B = 2
    xy = _batch(cfg, B, 6)
    tf = TorchCPUFlow(**kw)
    T = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in P.items()}
    ins, outs = [], []
    orig = tf._coupling

    def rec(u, c, PP, d):
        v, ld = orig(u, c, PP, d)
        v.retain_grad()
        ins.append(u.detach().numpy().copy())
        outs.append(v)
        return v, ld
    tf._coupling = rec
    try:
        tf.log_loss(torch.from_numpy(np.asarray(xy, np.float64)), T)[0].backward()
    finally:
        tf._coupling = orig
    flow = _gpu_flow(kw, P, gpu)
    layers = [L for L in flow.layers_list if hasattr(L, 'coupling_index')]
    couplings = [e.coupling for e in tf.layers if e.kind == 'coupling']
    assert len(layers) == len(couplings) == len(ins) == 16
    g_ld = -1.0 / B
    report = []
    for L, c, u, v in zip(layers, couplings, ins, outs):
        dv = v.grad.numpy()
        grads = {}
        for dt in (torch.float64, torch.float32):
            TT = {k: torch.tensor(np.asarray(x, np.float64), dtype=dt, requires_grad=True) for k, x in P.items()
                  if k.startswith(f'c{c.index}.')}
            ut = torch.tensor(u, dtype=dt, requires_grad=True)
            vv, ld = tf._coupling(ut, c, TT, +1)
            (torch.sum(vv * torch.from_numpy(dv).to(dt)) + g_ld * B * ld).backward()
            grads[dt] = ({k: t.grad.double().numpy().reshape(-1) for k, t in TT.items()}, ut.grad.double().numpy())
        (G, gu), (G32, gu32) = grads[torch.float64], grads[torch.float32]
        du, dp = L.gradients(torch.from_numpy(u).float().to(gpu), torch.from_numpy(dv).float().to(gpu), g_ld)
        du = du.cpu().numpy().astype(np.float64)
        dp = dp.cpu().numpy().astype(np.float64)
        gmax = max(float(np.max(np.abs(x))) for x in G.values())
        rel = 0.0
        for n, o, s in flow.param_specs:
            if n not in G:
                continue
            size = int(np.prod(s)) if s else 1
            err = float(np.max(np.abs(dp[o:o + size] - G[n])))
            tol = _tol(G[n], G32[n], gmax, K32_LAYER)
            rel = max(rel, err / tol)
            assert err <= tol, (c.index, n, err, tol)
        e_u = float(np.max(np.abs(du - gu)))
        tol_u = _tol(gu, gu32, 0.0, K32_LAYER)
        assert e_u <= tol_u, (c.index, e_u, tol_u)
        report.append(f'c{c.index}: du/tol {e_u / tol_u:.2f} dp/tol {rel:.2f}')
    print(' '.join(report))
