"""GPU (-m gpu): HRNet's input gradients, d lrs and d alphas (reference HRNet.py:198-204 and :113-132), through
hrn_hrnet_backward_in.

Oracle: fp64 torch autograd on the CPU through oracle/torch_port.hrnet_forward (tests/util._hrnet_forward_s at x2 / x4)
with lrs and alphas requiring grad.  The reference frame is the lower median of the first min(V, 9) views; torch.median's gradient goes
to the one index it returns, which torch leaves open among tied views (the zero padding views always tie).  So every oracle runs twice:
as is (torch's routing), and with the median's values as a separate leaf, which yields the stem's channel-0 gradient per view (c0) and
the reference frame's gradient (R) apart.  The HIP side must then
  - agree with torch's routing tie-invariantly: elementwise where the median is unique, summed over the tied views where it is not;
  - put R on exactly one view per pixel, the lowest-indexed tied one (the documented rule): c0 + R there, c0 elsewhere.
"""
import numpy as np
import pytest
import torch

from oracle import synth, torch_port, weights
import util
from util import _SLOPE_KEYS, _forward, _fresh_model, _model, _oracle, _real_median, _state, _tie_invariant_err

pytestmark = pytest.mark.gpu


def _check(got_lrs, got_alphas, lrs, alphas, cot, alpha_residual, slopes=None, scale=3, tol=2e-4):
    want_lrs, want_alphas, _ = _oracle(lrs, alphas, cot, alpha_residual, slopes, scale)
    c0, _, R = _oracle(lrs, alphas, cot, alpha_residual, slopes, scale, split=True)
    B, V = alphas.shape
    n = min(V, 9)
    med = _real_median(torch.from_numpy(lrs[:, :n]), 1).values.numpy()
    tied = lrs[:, :n] == med[:, None]                                   # (B, n, H, W)
    ntied = tied.sum(1)
    first = np.argmax(tied, 1)                                          # the lowest-indexed view equal to the median
    scale_l = max(np.abs(want_lrs).max(), 1e-30)
    # the documented rule, elementwise
    rule = c0.copy()
    np.put_along_axis(rule, first[:, None], np.take_along_axis(rule, first[:, None], 1) + R[:, None], 1)
    assert np.abs(got_lrs - rule).max() <= tol * scale_l, ("rule", np.abs(got_lrs - rule).max() / scale_l)
    # tie-invariantly against torch's own routing
    uniq = np.concatenate([np.broadcast_to(ntied[:, None] == 1, tied.shape), np.ones((B, V - n) + lrs.shape[2:], bool)], 1)
    assert np.abs(got_lrs - want_lrs)[uniq].max(initial=0.0) <= tol * scale_l
    sum_got = np.where(tied, got_lrs[:, :n], 0).sum(1)
    sum_want = np.where(tied, want_lrs[:, :n], 0).sum(1)
    assert np.abs(sum_got - sum_want).max() <= tol * scale_l * 9
    # views that are not tied with the median take channel 0 only
    assert np.abs(np.where(tied, 0, got_lrs[:, :n] - c0[:, :n])).max() <= tol * scale_l
    # ... and on the tied ones, R lands on exactly one
    hit = np.abs(got_lrs[:, :n] - c0[:, :n] - R[:, None]) <= tol * scale_l
    big = np.abs(R) > 10 * tol * scale_l
    assert (np.where(tied, hit, False).sum(1)[big] == 1).all()
    # d alphas
    if want_alphas is None:
        assert got_alphas is None
    else:
        assert got_alphas is not None
        err = np.abs(got_alphas - want_alphas)
        bound = 2e-5 * _abs_alpha_terms(lrs, alphas, cot, alpha_residual, slopes, scale) + 1e-12
        assert (err <= bound).all(), (err, bound)


def _abs_alpha_terms(lrs, alphas, cot, alpha_residual, slopes=None, scale=3):
    """sum over channels and pixels of |dsn * f| for each alpha entry: the terms of the sum that defines its gradient, in absolute
    value, from autograd on each level's product a_bob * f (recorded by a wrapper of Tensor.__mul__ during one fp64 forward)."""
    B, V = alphas.shape
    out = np.zeros((B, V))
    st = {k: v.double() for k, v in _state(scale, slopes=slopes).items()}
    recs = []
    orig_mul = torch.Tensor.__mul__

    def mul(self, other):
        y = orig_mul(self, other)
        if torch.is_tensor(other) and self.dim() == 5 and tuple(self.shape[2:]) == (1, 1, 1) and other.dim() == 5:
            recs.append((y, other))                                     # a_bob (B, half, 1, 1, 1) * f (B, half, 64, H, W)
        return y

    x = torch.from_numpy(lrs).double()
    a = torch.from_numpy(alphas).double().requires_grad_(True)
    try:
        torch.Tensor.__mul__ = mul
        with torch.enable_grad():
            sr = _forward(x, a, st, alpha_residual, scale)
    finally:
        torch.Tensor.__mul__ = orig_mul
    if not recs:
        return out
    gs = torch.autograd.grad((sr * torch.from_numpy(cot).double()).sum(), [r[0] for r in recs])
    n = V
    for (_, f), g in zip(recs, gs):
        half, parity = n // 2, n % 2
        t = (g * f).abs().sum(dim=(2, 3, 4)).detach().numpy()           # (B, half): bob j is view n - parity - 1 - j
        for j in range(half):
            out[:, n - parity - 1 - j] += t[:, j]
        n = half
    return out


def _run(prec, B, V, S, n_real, alpha_residual, slopes=None, scale=3, seed=5):
    lrs, alphas, _ = synth.make_batch(seed, B, V, S, n_real)
    rng = np.random.Generator(np.random.PCG64(77))
    cot = rng.standard_normal((B, 1, scale * S, scale * S)).astype(np.float32)
    m = _fresh_model(alpha_residual, precision=prec, slopes=slopes) if scale == 3 else \
        _model(scale, precision=prec, alpha_residual=alpha_residual, slopes=slopes, train=True)
    x, a = util.dev(lrs).requires_grad_(True), util.dev(alphas).requires_grad_(True)
    sr = m(x, a)
    (sr * util.dev(cot)).sum().backward()
    return lrs, alphas, cot, x.grad.cpu().numpy(), (None if a.grad is None else a.grad.cpu().numpy())


_GRID = [
    (2, 4, 16, 4, True),
    (2, 5, 16, 4, True),
    (1, 7, 24, 7, True),
    (2, 6, 16, 6, False),
    (2, 1, 16, 1, True),
    (1, 3, 33, 3, True),
    (2, 2, 5, 2, True),
    (1, 9, 37, 1, True),
    (1, 32, 16, 20, True),      # views beyond the median window, padded views beyond it; five fusion levels
]


@pytest.mark.parametrize("B,V,S,n_real,alpha_residual", _GRID)
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_input_grads_vs_autograd_oracle(B, V, S, n_real, alpha_residual, prec):
    """bf16x3, and V = 32 in both precisions, with every PReLU slope at 1 (see test_gpu_backward.test_hrnet_backward_vs_autograd_oracle:
    an activation near zero whose sign differs between the device's forward and the fp64 oracle moves the gradient behind it by
    O(1) at a few pixels; elementwise checks of d lrs see that, and five fusion levels at V = 32 give enough such activations even in
    fp32).  With slopes at 1 nothing can flip."""
    slopes = None if prec == "fp32" and V < 32 else {k: 1.0 for k in _SLOPE_KEYS}
    lrs, alphas, cot, g_lrs, g_alphas = _run(prec, B, V, S, n_real, alpha_residual, slopes)
    assert g_lrs.shape == lrs.shape
    _check(g_lrs, g_alphas, lrs, alphas, cot, alpha_residual, slopes)


@pytest.mark.parametrize("scale,B,V,S,n_real", [(2, 2, 5, 16, 4), (2, 1, 9, 33, 6), (4, 2, 4, 16, 4), (4, 1, 7, 24, 5)])
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_input_grads_at_x2_x4(scale, B, V, S, n_real, prec):
    slopes = None if prec == "fp32" else {k: 1.0 for k in _SLOPE_KEYS}
    lrs, alphas, cot, g_lrs, g_alphas = _run(prec, B, V, S, n_real, True, slopes, scale=scale, seed=23)
    _check(g_lrs, g_alphas, lrs, alphas, cot, True, slopes, scale=scale)


def test_full_train_step_input_grad_vs_autograd_oracle():
    """d loss / d lrs (and d alphas) through HRNet -> ShiftNet -> Lanczos -> get_loss (train.py:172-190) against torch_port.train_step
    in fp64.  The chain is ill-conditioned in fp32 (see test_gpu_backward.test_full_train_step_vs_autograd_oracle): 2e-2 of the
    max-norm, where torch's own fp32 autograd is 3e-3..7e-3 off."""
    from DeepNetworks.ShiftNet import ShiftNet
    B, V, S, lam = 2, 3, 48, 1e-6
    lrs, alphas, hrs = synth.make_batch(31, B, V, S, V)
    rng = np.random.Generator(np.random.PCG64(5))
    maps = (rng.random((B, 3 * S, 3 * S)) > 0.1).astype(np.float32)
    mask = rng.random((B, 32768)) >= 0.5
    hst = {k: v.double() for k, v in weights.to_torch_state(weights.hrnet_state(1234)).items()}
    sstate = weights.to_torch_state(weights.shiftnet_state(4321))
    sst = {k: v.double() for k, v in sstate.items()}
    x = torch.from_numpy(lrs).double().requires_grad_(True)
    a = torch.from_numpy(alphas).double().requires_grad_(True)
    with torch.enable_grad():
        loss, _, _, _ = torch_port.train_step(x, a, torch.from_numpy(hrs).double(), torch.from_numpy(maps).double(),
                                              torch.from_numpy(mask).double(), hst, sst, lam=lam)
        loss.backward()
    crop = np.ones((3 * S, 3 * S), np.float32)
    crop[:3] = 0; crop[-3:] = 0; crop[:, :3] = 0; crop[:, -3:] = 0
    off = (3 * S - 128) // 2
    fusion = _fresh_model(True)
    regis = ShiftNet()
    regis.load_state_dict(sstate)
    regis = regis.cuda().train()
    g_x, g_a, d_hrs = util.dev(lrs).requires_grad_(True), util.dev(alphas).requires_grad_(True), util.dev(hrs)
    dmask = torch.from_numpy(mask.astype(np.uint8)).cuda()
    orig_rand = torch.rand
    try:
        torch.rand = lambda *s, **k: (dmask.float() * 0.75 + 0.125).reshape(s[0]) if s and tuple(s[0]) == (B, 32768) else orig_rand(*s, **k)
        g_srs = fusion(g_x, g_a)
        g_shifts = util._register_batch(regis, g_srs[:, :, off:off + 128, off:off + 128],
                                      d_hrs[:, off:off + 128, off:off + 128].reshape(-1, 1, 128, 128))
        bsz, nv, hh, ww = g_srs.shape
        g_shifted = regis.transform(g_shifts.view(-1, 2), g_srs.view(-1, 1, hh, ww), device="cuda").view(-1, nv, hh, ww)[:, 0]
    finally:
        torch.rand = orig_rand
    g_loss = -util._get_loss_cpsnr(g_shifted, d_hrs, util.dev(crop * maps))
    g_loss = g_loss.mean() + lam * g_shifts.mean() ** 2
    g_loss.backward()
    assert abs(float(g_loss.detach()) - float(loss.detach())) <= 2e-4 * abs(float(loss.detach()))
    assert g_x.grad is not None and g_a.grad is not None
    err = _tie_invariant_err(g_x.grad.cpu().numpy(), x.grad.numpy(), lrs)
    assert err <= 2e-2, err
    assert util.rel_err(g_a.grad.cpu().numpy(), a.grad.numpy()) <= 2e-2, (g_a.grad, a.grad)


def _train_shape_grads(prec, want_inputs, seed=3, slopes=None):
    B, V, S = 32, 32, 64
    lrs, alphas, _ = synth.make_batch(seed, B, V, S, [32 - (b % 9) for b in range(B)])
    cot = np.random.Generator(np.random.PCG64(9)).standard_normal((B, 1, 3 * S, 3 * S)).astype(np.float32)
    m = _fresh_model(True, precision=prec, slopes=slopes)
    x, a = util.dev(lrs), util.dev(alphas)
    if want_inputs:
        x.requires_grad_(True); a.requires_grad_(True)
    (m(x, a) * util.dev(cot)).sum().backward()
    params = {k: p.grad.cpu().numpy() for k, p in m.named_parameters()}
    out = (x.grad.cpu().numpy(), a.grad.cpu().numpy()) if want_inputs else (None, None)
    del m, x, a
    torch.cuda.empty_cache()
    return out, params


def test_input_grads_at_train_shape():
    """B=32, V=32, 64 x 64 (the bench's training shape): two runs bit-identical; parameter gradients bit-identical whether or not the
    input gradients were asked for, in both precisions; bf16x3 input gradients against fp32's (below)."""
    (l32, a32), p32 = _train_shape_grads("fp32", True)
    (l32b, a32b), _ = _train_shape_grads("fp32", True)
    assert np.array_equal(l32, l32b) and np.array_equal(a32, a32b)
    _, p32n = _train_shape_grads("fp32", False)
    assert all(np.array_equal(p32[k], p32n[k]) for k in p32)
    (lx3, ax3), px3 = _train_shape_grads("bf16x3", True)
    (lx3b, ax3b), _ = _train_shape_grads("bf16x3", True)
    assert np.array_equal(lx3, lx3b) and np.array_equal(ax3, ax3b)
    _, px3n = _train_shape_grads("bf16x3", False)
    assert all(np.array_equal(px3[k], px3n[k]) for k in px3)
    assert np.isfinite(a32).all() and np.abs(a32).max() > 0
    # bf16x3 against fp32.  With every slope at 1 nothing can flip sign: elementwise 2e-4 of the max-norm.  At the default slopes the
    # near-zero activations that take the other sign in one of the two forwards (~1e-5 apart) move d lrs by O(1) at the pixels behind
    # them; per-pixel gradients do not average that out as the weight gradients do (measured: mean 4.6e-5, 99.9th percentile 1.7e-3,
    # max 1.6e-2 of the max-norm), so there the mean is held to 1e-4 and the maximum to 5e-2.
    ones = {k: 1.0 for k in _SLOPE_KEYS}
    (l1, a1), _ = _train_shape_grads("fp32", True, slopes=ones)
    (lx1, ax1), _ = _train_shape_grads("bf16x3", True, slopes=ones)
    assert util.rel_err(lx1, l1) <= 2e-4, util.rel_err(lx1, l1)
    e = np.abs(lx3 - l32) / np.abs(l32).max()
    assert e.mean() <= 1e-4 and e.max() <= 5e-2, (e.mean(), e.max())
    assert util.rel_err(ax1, a1) <= 2e-4, util.rel_err(ax1, a1)


def test_routing_eval_frozen_and_bf16():
    """Grad enabled and lrs / alphas requiring grad: the training forward of the module's precision in either mode, frozen parameters
    included; the output equals the inference kernels'.  Precision "bf16" returns its fp32 recompute's input gradients."""
    lrs, alphas, _ = synth.make_batch(5, 2, 5, 16, 4)
    cot = util.dev(np.random.Generator(np.random.PCG64(77)).standard_normal((2, 1, 48, 48)).astype(np.float32))
    ref_in = {}
    # (bf16x3: the training and the inference kernels are each ~1e-5 from the fp64 forward, so up to ~2e-5 from each other)
    for prec, tol in (("fp32", 1e-6), ("bf16x3", 4e-5)):
        m = _fresh_model(True, precision=prec)
        x, a = util.dev(lrs).requires_grad_(True), util.dev(alphas).requires_grad_(True)
        (m(x, a) * cot).sum().backward()
        ref_in[prec] = (x.grad.clone(), a.grad.clone())
        m.eval()
        with torch.no_grad():
            inf = m(util.dev(lrs), util.dev(alphas))
        m.zero_grad(set_to_none=True)
        x, a = util.dev(lrs).requires_grad_(True), util.dev(alphas).requires_grad_(True)
        sr = m(x, a)
        assert sr.grad_fn is not None
        assert util.rel_err(sr.detach().cpu().numpy(), inf.cpu().numpy()) <= tol
        (sr * cot).sum().backward()
        assert torch.equal(x.grad, ref_in[prec][0]) and torch.equal(a.grad, ref_in[prec][1])
        assert all(p.grad is not None for p in m.parameters())          # eval mode, parameters requiring grad: they get theirs too
        # frozen parameters: no parameter .grad, same input gradients
        m.requires_grad_(False)
        m.zero_grad(set_to_none=True)
        x, a = util.dev(lrs).requires_grad_(True), util.dev(alphas)
        (m(x, a) * cot).sum().backward()
        assert torch.equal(x.grad, ref_in[prec][0])
        assert all(p.grad is None for p in m.parameters())
    # bf16: inference kernels forward (bit-identical output), fp32 recompute's gradients
    m = _fresh_model(True, precision="bf16").eval()
    with torch.no_grad():
        inf = m(util.dev(lrs), util.dev(alphas))
    x, a = util.dev(lrs).requires_grad_(True), util.dev(alphas).requires_grad_(True)
    sr = m(x, a)
    assert torch.equal(sr.detach(), inf)
    with pytest.warns(RuntimeWarning):
        from DeepNetworks.HRNet import _HRNetLazyTrainFunction
        _HRNetLazyTrainFunction._warned = False
        (sr * cot).sum().backward()
    assert torch.equal(x.grad, ref_in["fp32"][0]) and torch.equal(a.grad, ref_in["fp32"][1])


def test_opcheck_backward_in():
    from hrnet_hip import binding
    lrs, alphas, _ = synth.make_batch(5, 1, 4, 8, 4)
    m = _fresh_model(True)
    params = [p.detach() for p in m.parameters()]
    packed = m._packed_f32()
    x, a = util.dev(lrs), util.dev(alphas)
    _, tws = torch.ops.hrnet_hip.hrnet_forward_train(packed, x, a, params, 2, True, binding.F32, 3)
    d_sr = torch.randn((1, 1, 24, 24), device="cuda")
    for need_l, need_a in ((True, True), (True, False), (False, True)):
        torch.library.opcheck(torch.ops.hrnet_hip.hrnet_backward_in.default,
                              (packed, params, x, a, d_sr, tws, 2, True, binding.F32, 3, need_l, need_a),
                              test_utils=("test_schema", "test_faketensor"))
