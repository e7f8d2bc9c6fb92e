"""CPU: the fp64 references of tests/test_gpu_kernels_shiftnet.py against torch (float64) - autograd of the forward operation each belongs to,
torch.optim.Adam for the optimiser - and the claims that file makes about its own inputs: ties and all-non-positive windows present, exact
zeros present, `x * scale + shift` and the operand products exact in fp32, the high-mean and constant channels of the statistics inputs,
the n_seq values, and the Adam bounds on a float32 restatement of the kernel's formula."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kernel_refs as K
from kernel_bounds import _exact_affine, _quantised

D = torch.float64


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=D) * scale


def _close(got, want, tol=1e-12):
    assert got.shape == want.shape, (got.shape, want.shape)
    assert float((got - want).abs().max()) <= tol * (1.0 + float(want.abs().max())), float((got - want).abs().max())


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


# ----------------------------------------------------------------------------------------------------------- BatchNorm
def test_bn_stats_reference():
    """F.batch_norm in train mode: its output is x scale + shift, its running statistics those of ref_bn_stats; the two wrong variants differ"""
    npix, Cc = 257, 64
    x = _rand((npix, Cc), 1) * 0.7 + torch.linspace(-1, 1, Cc, dtype=D)
    gamma, beta, rm0, rv0 = _rand((Cc,), 2), _rand((Cc,), 3), _rand((Cc,), 4), _rand((Cc,), 5).abs() + 0.5
    rm, rv = rm0.clone(), rv0.clone()
    out = F.batch_norm(x.T.reshape(1, Cc, npix, 1), rm, rv, gamma, beta, training=True, momentum=K.MOM, eps=K.EPS)
    ref = K.ref_bn_stats(x, gamma, beta, rm0, rv0)
    _close(x * ref["scale"][0] + ref["shift"][0], out.reshape(Cc, npix).T, 1e-11)
    _close(ref["running_mean"][0], rm)
    _close(ref["running_var"][0], rv)
    _close(ref["mean"][0], x.mean(0))
    _close(ref["invstd"][0], 1.0 / torch.sqrt(x.var(0, unbiased=False) + K.EPS))
    for k, (v, T) in ref.items():
        assert bool((T >= v.abs() - 1e-12).all()), k
    assert float((K.ref_bn_stats(x, gamma, beta, rm0, rv0, unbiased_scale=True)["scale"][0] - ref["scale"][0]).abs().max()) > 1e-4
    assert float((K.ref_bn_stats(x, gamma, beta, rm0, rv0, biased_running=True)["running_var"][0] - rv).abs().max()) > 1e-5


@pytest.mark.parametrize("dt", [K.F32, K.BF16])
@pytest.mark.parametrize("npix", list(K.BN_NPIX.values()))
def test_bn_stats_inputs(npix, dt):
    """the statistics inputs: a channel with mean^2 / var >= HIGH[dt], three exactly constant channels, bf16 values representable; and
    the kernel's formula (ss / n - mean^2 in fp64, then 1 / sqrtf((float)var + eps)) is within C of torch's fp64 two-pass variance on
    them, with the variance of the constant channels clamped to 0 or negligible against eps"""
    x, gamma, *_ = K.bn_stats_inputs(npix, 64, dt, 7 + 64 + npix % 1000)
    if dt == K.BF16:
        assert torch.equal(x.to(torch.bfloat16).float(), x)
    x = x.double()
    mean, var = x.mean(0), x.var(0, unbiased=False)
    assert float((mean[3:5] ** 2 / var[3:5]).max()) >= K.HIGH[dt]
    assert all(bool((x[:, c] == x[0, c]).all()) for c in (5, 6, 7)) and float(var[5:8].max()) <= 1e-30
    assert bool((gamma > 0).any()) and bool((gamma < 0).any())
    n = float(npix)
    m = x.sum(0) / n
    v = ((x * x).sum(0) / n - m * m).clamp_min(0.0)
    assert float(v[5:8].max()) <= 1e-12 * K.EPS
    istd = 1.0 / torch.sqrt(v.float() + np.float32(1e-5))
    want = 1.0 / torch.sqrt(var + K.EPS)
    worst = float(((istd.double() - want).abs() / want).max())
    print(f"npix {npix}: invstd of the one-pass formula against the two-pass fp64 one: {worst:.2e}")
    assert worst <= K.C


@pytest.mark.parametrize("bias", [True, False])
def test_bn_fold_reference(bias):
    """eval-mode BatchNorm2d(conv_nobias + conv_bias) == conv_nobias scale + shift"""
    Cc = 64
    y = _rand((3, Cc, 4, 5), 6)
    gamma, beta, rm, rv, cb = _rand((Cc,), 7), _rand((Cc,), 8), _rand((Cc,), 9), _rand((Cc,), 10).abs() + 0.1, _rand((Cc,), 11)
    want = F.batch_norm(y + (cb.view(1, -1, 1, 1) if bias else 0), rm, rv, gamma, beta, training=False, eps=K.EPS)
    (sc, Ts), (sh, Th) = K.ref_bn_fold(gamma, beta, rm, rv, cb if bias else None)
    _close(y * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1), want)
    assert bool((Ts >= sc.abs()).all()) and bool((Th >= sh.abs() - 1e-12).all())


@pytest.mark.parametrize("pool", [0, 1])
def test_bn_act_pool_reference(pool):
    N, H, Cc = 2, 8, 64
    x, sc, sh = _rand((N, H, H, Cc), 12), _rand((Cc,), 13), _rand((Cc,), 14)
    v = F.relu(K._nchw(x) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    want = _nhwc(F.max_pool2d(v, 2) if pool else v)
    got, T = K.ref_bn_act_pool(x, sc, sh, pool)
    _close(got, want)
    assert bool((T >= got - 1e-12).all())
    got, _ = K.ref_bn_act_pool(x, None, None, pool)
    _close(got, _nhwc(F.max_pool2d(F.relu(K._nchw(x)), 2) if pool else F.relu(K._nchw(x))))
    w = K._windows(x)
    assert torch.equal(K._unwindows(w), x) and torch.equal(w[0, 1, 2, 3], torch.stack([x[0, 2, 4, 3], x[0, 2, 5, 3], x[0, 3, 4, 3], x[0, 3, 5, 3]]))


@pytest.mark.parametrize("pool", [0, 1])
def test_bn_bwd_reference(pool):
    """BatchNorm2d (train) + ReLU + MaxPool2d(2) in fp64 on quantised x: tied windows are common, and torch routes a tied window's gradient
    to its first maximum in row-major order, as ref_bn_dv does; last-maximum routing differs"""
    N, H, Cc = 3, 16, 64
    x0 = _quantised((N, H, H, Cc), 15)
    gamma0, beta0 = _rand((Cc,), 16) + 0.2, _rand((Cc,), 17) * 0.3
    x = K._nchw(x0).contiguous().requires_grad_(True)
    gamma, beta = gamma0.clone().requires_grad_(True), beta0.clone().requires_grad_(True)
    v = F.relu(F.batch_norm(x, None, None, gamma, beta, training=True, eps=K.EPS))
    y = F.max_pool2d(v, 2) if pool else v
    dy = _rand(tuple(_nhwc(y).shape), 18)
    (_nhwc(y) * dy).sum().backward()
    st = K.ref_bn_stats(x0.reshape(-1, Cc), gamma0, beta0, None, None)
    args = (x0, dy, st["mean"][0], st["invstd"][0], st["scale"][0], st["shift"][0], gamma0, pool)
    if pool:
        tied, dead = K._window_counts(_nhwc(v.detach()))
        assert tied > 100 and dead > 10, (tied, dead)
    ref = K.ref_bn_bwd(*args)
    _close(ref["dx"][0], _nhwc(x.grad), 1e-10)
    _close(ref["dgamma"][0], gamma.grad, 1e-10)
    _close(ref["dbeta"][0], beta.grad, 1e-10)
    for k, (val, T) in ref.items():
        assert bool((T >= val.abs() - 1e-9).all()), k
    if pool:
        assert float((K.ref_bn_bwd(*args, last_max=True)["dx"][0] - _nhwc(x.grad)).abs().max()) > 1e-3


@pytest.mark.parametrize("Cc,H,pool", [(64, 32, 0), (64, 32, 1), (128, 16, 0), (128, 16, 1)])
def test_exact_affine_inputs(Cc, H, pool):
    """the quantised x with a power-of-two scale and a coarse shift: x scale + shift evaluated in fp32 (either as a product and a sum or fused)
    is the fp64 value; both storages hold x exactly; the windows of the GPU cases hold ties, all-non-positive windows and exact zeros"""
    for seed in (7 + Cc + pool, 11 + Cc + pool):
        x = _quantised((3, H, H, Cc), seed)
        sc, sh = _exact_affine(Cc, seed + 1)
        assert torch.equal(x.float().to(torch.bfloat16).double(), x)
        v64 = x * sc.double() + sh.double()
        assert torch.equal((x.float() * sc + sh).double(), v64) and torch.equal(torch.addcmul(sh.expand_as(x), x.float(), sc.expand_as(x)).double(), v64)
        r = torch.relu(v64)
        tied, dead = K._window_counts(r)
        assert tied > 100 and dead > 100 and bool((r == 0).any()) and bool((r > 0).any())


# ----------------------------------------------------------------------------------------------------------- convolutions, plane mean
def test_conv_bn_relu_reference():
    """ReLU(BatchNorm2d.eval()(Conv2d(x))) with the fold of ref_bn_fold"""
    M, H, W, cin, cout = 2, 5, 7, 64, 128
    x, w, cb = _rand((M, H, W, cin), 19), _rand((cout, cin, 3, 3), 20) * 0.05, _rand((cout,), 21)
    gamma, beta, rm, rv = _rand((cout,), 22), _rand((cout,), 23), _rand((cout,), 24), _rand((cout,), 25).abs() + 0.1
    want = F.relu(F.batch_norm(F.conv2d(K._nchw(x), w, cb, padding=1), rm, rv, gamma, beta, training=False, eps=K.EPS))
    (sc, _), (sh, _) = K.ref_bn_fold(gamma, beta, rm, rv, cb)
    got, T = K.ref_conv_bn_relu(x, w, sc, sh)
    _close(got, want)
    assert bool((T >= got - 1e-12).all())


def test_plane_mean_backward():
    """x - x.mean((2, 3)): its backward is g - mean(g) per plane, what plane_mean_kernel + sub_plane_mean_kernel compute"""
    x = _rand((3, 2, 5, 7), 26).requires_grad_(True)
    g = _rand((3, 2, 5, 7), 27)
    ((x - x.mean((2, 3), keepdim=True)) * g).sum().backward()
    _close(g - g.mean((2, 3), keepdim=True), x.grad)


def test_stem_dgrad_reference():
    M, H, W = 5, 4, 6
    x = _rand((M, 2, H, W), 28).requires_grad_(True)
    w = _rand((64, 2, 3, 3), 29) * 0.2
    g = _rand((M, H, W, 64), 30)
    (F.conv2d(x, w, None, padding=1) * K._nchw(g)).sum().backward()
    got, T = K.ref_stem_dgrad(g, w, step=2)
    _close(got, x.grad)
    _close(got, F.conv_transpose2d(K._nchw(g), w, padding=1))
    assert bool((T >= got.abs() - 1e-12).all())


# ----------------------------------------------------------------------------------------------------------- the fully connected tail
@pytest.mark.parametrize("masked", [False, True])
def test_fc_tail_references(masked):
    """theta = fc2(ReLU(fc1(dropout(flatten(y))))) with the reference's (C, H, W) flatten order of an NHWC y and the dropout mask with kept
    activations x 2 (a 16-neuron fc1: the references take the weight's row count from the tensor)"""
    B, J = 3, 16
    y = _rand((B, 256, 128), 31).requires_grad_(True)                       # NHWC, hw = 16 x 16
    mask = K._mask(B, 32) if masked else None
    w1, b1, w2 = (_rand((J, K.FCK), 33) * 0.01).requires_grad_(True), _rand((J,), 34).requires_grad_(True), _rand((2, J), 35).requires_grad_(True)
    h = y.reshape(B, 16, 16, 128).permute(0, 3, 1, 2).reshape(B, -1)        # the module's x.view(-1, 128 * 16 * 16) of an NCHW tensor
    if masked:
        h = h * mask.double() * 2.0
    h.retain_grad()
    z1 = F.linear(h, w1, b1)
    z1.retain_grad()
    y1 = F.relu(z1)
    theta = F.linear(y1, w2)
    dth = _rand((B, 2), 36)
    (theta * dth).sum().backward()
    xr = K.ref_fc_to_ref(y.detach(), mask)
    _close(xr, h.detach())
    got, T = K.ref_fc1(xr, w1.detach().float().double(), b1.detach(), block=5)
    _close(got, F.relu(F.linear(xr, w1.detach().float().double(), b1.detach())))
    _close(K.ref_fc1(xr, w1.detach(), b1.detach())[0], y1.detach())
    _close(K.ref_fc2(y1.detach(), w2.detach())[0], theta.detach())
    ref = K.ref_fc2_bwd(dth, y1.detach(), w2.detach())
    assert bool((y1 == 0).any())
    _close(ref["dz1"][0], z1.grad)
    _close(ref["dw2"][0], w2.grad)
    _close(ref["db1"][0], b1.grad)
    assert float((K.ref_fc2_bwd(dth, y1.detach(), w2.detach(), gate_ge=True)["dz1"][0] - z1.grad).abs().max()) > 1e-3
    _close(K.ref_fc1_bwd_w(z1.grad, xr, 0, J)[0], w1.grad)
    _close(K.ref_fc1_bwd_w(z1.grad, xr, 3, 7)[0], w1.grad[3:7])
    dxr, T = K.ref_fc1_bwd_x(z1.grad, w1.detach(), block=5)
    _close(dxr, h.grad)
    _close(K.ref_fc_from_ref(dxr, mask), y.grad)
    assert bool((T >= dxr.abs() - 1e-12).all())
    # the wrong variants of the negative controls differ
    assert float((K.ref_fc_to_ref(y.detach(), mask, hwc=True) - h.detach()).abs().max()) > 1e-3
    if masked:
        assert float((K.ref_fc_to_ref(y.detach(), mask, keep=1.0) - h.detach()).abs().max()) > 1e-3


def test_fc1_group_shift_reference():
    xr = _rand((33, 64), 37)
    w, b = _rand((8, 64), 38), _rand((8,), 39)
    right, _ = K.ref_fc1(xr, w, b)
    wrong, _ = K.ref_fc1(xr, w, b, shift_group=True)
    assert torch.equal(right[:32], wrong[:32]) and torch.equal(wrong[32], right[0]) and not torch.equal(wrong[32], right[32])


def test_products_exact_and_n_seq():
    """bf16-representable operands (and 16 significant bits against 8) multiply exactly in fp32; the chain lengths the GPU file derives its
    constants from"""
    a, b = K.rnd((4096,), 1, K.BF16), K.rnd((4096,), 2, K.BF16) * 0.125
    assert torch.equal(a.to(torch.bfloat16).float(), a) and torch.equal(b.to(torch.bfloat16).float(), b)
    assert torch.equal((a * b).double(), a.double() * b.double())
    q = K.rnd((4096,), 3, K.F32)                                         # 16 significant bits
    assert torch.equal((q * b).double(), q.double() * b.double())
    w = K._stem_dgrad_w(51)
    assert torch.equal(w.to(torch.bfloat16).float(), w) and torch.equal((q[:1152].reshape(64, 2, 3, 3) * w).double(), q[:1152].reshape(64, 2, 3, 3).double() * w.double())
    assert K.FC1_NSEQ == (4096 // 256) * 64 + 8 * 4 + 1 == 1057        # FC_NST stages x 64 k per wave, FC_SPLIT slabs, the bias
    assert K.FCX_NSEQ == 128 * 2 + 3 == 259                             # 128 steps x 2 j per wave, three additions of the waves' sums
    assert max(K.C, 9 * 64 * 2.0 ** -24) == 9 * 64 * 2.0 ** -24 and 65 <= 128


# ----------------------------------------------------------------------------------------------------------- Adam
@pytest.mark.parametrize("si", range(len(K.ADAM_SETTINGS)))
def test_adam_reference(si):
    """torch.optim.Adam in float64 over five steps (its step counter starts where the setting says)"""
    lr, b1, b2, wd, step0 = K.ADAM_SETTINGS[si]
    p0, g0, m0, v0 = [t.double() for t in K.adam_inputs(1027, 40 + si)]
    p = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=K.ADAM_EPS, weight_decay=wd)
    opt.state[p] = dict(step=torch.tensor(float(step0 - 1)), exp_avg=m0.clone(), exp_avg_sq=v0.clone())
    rp, rm, rv = p0, m0, v0
    for k in range(5):
        g = g0 * (1.0 + 0.3 * k)
        p.grad = g.clone()
        opt.step()
        rm, _, rv, _, rp, _ = K.ref_adam(rp, g, rm, rv, lr, b1, b2, K.ADAM_EPS, wd, step0 + k)
        _close(rp, p.detach(), 1e-11)
        _close(rm, opt.state[p]["exp_avg"])
        _close(rv, opt.state[p]["exp_avg_sq"])
    wrong = K.ref_adam(p0, g0, m0, v0, lr, b1, b2, K.ADAM_EPS, wd, step0, no_bc2=True)[4]
    right = K.ref_adam(p0, g0, m0, v0, lr, b1, b2, K.ADAM_EPS, wd, step0)[4]
    if step0 < 1000:        # (1 - beta2^1000 = 0.63: the correction is small but there)
        assert float((wrong - right).abs().max()) > 1e-4
    assert float((K.ref_adam(p0, g0, m0, v0, lr, b1, b2, K.ADAM_EPS, wd, step0, eps_inside=True)[4] - right).abs().max()) > 1e-6


@pytest.mark.parametrize("si", range(len(K.ADAM_SETTINGS)))
def test_adam_bounds_on_float32_restatement(si):
    """the kernel's formula restated in float32 on the CPU meets the three bounds the GPU test holds the kernel to (so they come from the
    format, not from the kernel); the inputs hold g = 0, v = 0, m = 0 and g = 1e-30 elements, and 1 - beta is exact in fp32"""
    lr, b1, b2, wd, step = K.ADAM_SETTINGS[si]
    n = 200003
    p, g, m, v = K.adam_inputs(n, 130 + n % 1000)
    assert bool((g == 0).any()) and bool((v == 0).any()) and bool((m == 0).any()) and bool((g == 1e-30).any()) and bool((v >= 0).all())
    f = np.float32
    assert float(f(1) - f(b1)) == 1.0 - float(f(b1)) and float(f(1) - f(b2)) == 1.0 - float(f(b2))
    step_size = torch.tensor(float(f(float(f(lr)) / (1.0 - float(f(b1)) ** step))))
    inv_bc2 = torch.tensor(float(f(1.0 / np.sqrt(1.0 - float(f(b2)) ** step))))
    tb1, tb2, twd, teps = [torch.tensor(float(f(h))) for h in (b1, b2, wd, K.ADAM_EPS)]
    gj = g + twd * p
    m1 = tb1 * m + (1 - tb1) * gj
    v1 = tb2 * v + (1 - tb2) * gj * gj
    p1 = p - step_size * m1 / (torch.sqrt(v1) * inv_bc2 + teps)
    assert p1.dtype == torch.float32
    hyper = [float(f(h)) for h in (lr, b1, b2, K.ADAM_EPS, wd)] + [step]
    ins = [t.double() for t in (p, g, m, v)]
    wm, Tm, wv, Tv, _, _ = K.ref_adam(*ins, *hyper)
    rm = float(((m1.double() - wm).abs() / (K.C * Tm + 1e-300)).max())
    rv = float(((v1.double() - wv).abs() / (K.C * Tv + 2.0 ** -126)).max())
    rp = float(K._adam_p_ratio(dict(p=p1.double(), m=m1.double(), v=v1.double(), ins=ins, hyper=hyper)).max())
    print(f"setting {K.ADAM_SETTINGS[si]}: error / bound m' {rm:.3f}, v' {rv:.3f}, p' {rp:.3f}")
    assert rm <= 1.0 and rv <= 1.0 and rp <= 1.0
