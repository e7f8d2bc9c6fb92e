"""GPU (-m gpu): HRNet's `base=` - with `global_residual` on, a frame given by the caller takes the place of up(frame): every forward returns
net(...) + base, the base added once, where the skip is added.

  sum        with base = upsample(frame) the result is within one rounding of the sum of the fused skip (the comparison
             tests/test_gpu_upsample.py makes for torch's add); with any base it is plain forward + base, bit for bit, (B,SH,SW) and
             (B,1,SH,SW) alike, with `ref` keeping its own meaning
  paths      forward_tiled(base=) and forward_ensemble(base=) are bit-identical to forward(base=) wherever both exist, and to their own
             plain results plus the base elsewhere (a rectangular scene)
  training   parameter gradients bit-identical to the flag off, d_base == d_sr, lrs may require grad (nothing is taken as data)
  errors     base= without the flag raises, in all three forwards; a wrong shape, type or device raises
  None       base=None keeps today's bits (the fused skip) - and a shift-and-add frame goes in as the base
"""
import copy

import numpy as np
import pytest
import torch

import kt
import util
from hrnet_hip import composite, shiftadd, upsample
from oracle import synth, weights
from util import _state

pytestmark = pytest.mark.gpu

PRECS = ["fp32", "bf16", "bf16x3"]


def _build(scale, prec, flag=None, train=False, train_precision=None):
    from DeepNetworks.HRNet import HRNet
    cfg = copy.deepcopy(weights.HRNET_CONFIG)
    cfg["decoder"]["deconv"]["kernel_size"] = cfg["decoder"]["deconv"]["stride"] = scale
    if flag is not None:
        cfg["global_residual"] = flag
    m = HRNet(cfg)
    m.load_state_dict(_state(scale))
    m.precision, m.train_precision = prec, train_precision
    m = m.cuda()
    return m.train() if train else m.eval()


def _median(x):
    B, V, H, W = x.shape
    med = torch.empty((B, H, W), dtype=torch.float32, device="cuda")
    assert kt.lib().hrn_kt_median(kt._p(x), kt._p(med), B, V, H, W, kt._stream()) == 0
    return med


def _batch(seed, B, V, S):
    lrs, alphas, _ = synth.make_batch(seed, B, V, S, [V, max(1, V - 1)][:B] if B <= 2 else V)
    return util.dev(lrs), util.dev(alphas)


def _rand(shape, seed):
    return util.dev(np.random.Generator(np.random.PCG64(seed)).standard_normal(tuple(shape)).astype(np.float32))


@pytest.mark.parametrize("scale", [2, 3, 4])
@pytest.mark.parametrize("prec", PRECS)
def test_forward_with_a_base_is_the_plain_forward_plus_the_base(prec, scale):
    x, a = _batch(5 + scale, 2, 4, 16)
    off, on = _build(scale, prec), _build(scale, prec, True)
    with torch.no_grad():
        plain, fused = off(x, a), on(x, a)
        # the upsampled frame as the base: within one rounding of the fused skip's sum
        up = upsample.upsample(_median(x), scale)
        got = on(x, a, base=up)
        assert got.dtype == torch.float32 and not got.requires_grad and tuple(got.shape) == tuple(plain.shape)
        err = (got.double() - fused.double()).abs()
        print(f"{prec} x{scale}: max |forward(base=up) - fused skip| / |sum| = {float((err / fused.double().abs().clamp_min(1e-300)).max()):.3e}")
        assert bool((err <= 2.0 ** -23 * fused.double().abs()).all()) and not torch.equal(got, plain)
        # any base, in both shapes; the call leaves nothing behind in the unflagged model's output or in the base
        base = _rand(up.shape, 3)
        keep = base.clone()
        assert torch.equal(on(x, a, base=base), plain + base.unsqueeze(1))
        assert torch.equal(on(x, a, base=base.unsqueeze(1)), plain + base.unsqueeze(1))
        assert torch.equal(base, keep) and torch.equal(off(x, a), plain)
        # base=None is the fused skip it was
        assert torch.equal(on(x, a, base=None), fused) and torch.equal(on(x, a), fused)
        # ref keeps its meaning: the stem's frame, not the skip's
        ref, filled = composite.masked_composite(x, util.dev((np.random.Generator(np.random.PCG64(8)).random(tuple(x.shape)) < 0.6).astype(np.float32)), a)
        assert torch.equal(on(filled, a, ref=ref, base=base), off(filled, a, ref=ref) + base.unsqueeze(1))


@pytest.mark.parametrize("prec", PRECS)
def test_ensemble_and_tiled_add_the_base_once_and_agree_with_forward(prec):
    off, on = _build(3, prec), _build(3, prec, True)
    x, a = _batch(304 + 56, 2, 4, 56)
    base = _rand((2, 168, 168), 4)
    with torch.no_grad():
        whole = on(x, a, base=base)
        assert torch.equal(whole, off(x, a) + base.unsqueeze(1))
        # a square scene: the tiled result is the whole-frame forward, with the base as without
        assert torch.equal(on.forward_tiled(x, a, 32, base=base), whole) and torch.equal(on.forward_tiled(x, a, 56, base=base), whole)
        for mode in ("flip", "dihedral"):
            ens = on.forward_ensemble(x, a, mode, base=base)
            assert torch.equal(ens, off.forward_ensemble(x, a, mode) + base.unsqueeze(1))
            assert torch.equal(on.forward_tiled(x, a, 56, ensemble=mode, base=base), ens)
        assert torch.equal(on.forward_tiled(x, a, 32, ensemble="flip", base=base), on.forward_ensemble(x, a, "flip", base=base))
        assert torch.equal(on.forward_ensemble(x, a, "flip", members_per_pass=3, base=base.unsqueeze(1)), on.forward_ensemble(x, a, "flip", base=base))
        on.ensemble = "flip"                                     # the attributes route forward through the same sums: still one add
        assert torch.equal(on(x, a, base=base), on.forward_ensemble(x, a, "flip", base=base))
        on.ensemble = None
        # a rectangular scene (2, 4, 48, 40) in windows of 32
        rect = util.dev(synth.fast_batch(3, 2, 4, 48)[0][:, :, :, :40])
        ar = torch.ones(2, 4, device="cuda")
        rbase = _rand((2, 144, 120), 5)
        want = off.forward_tiled(rect, ar, 32) + rbase.unsqueeze(1)
        assert torch.equal(on.forward_tiled(rect, ar, 32, base=rbase), want)
        assert torch.equal(on.forward_tiled(rect, ar, 32, windows_per_pass=1, base=rbase), want)
        on.tile = 32
        assert torch.equal(on(rect, ar, base=rbase), want)
        on.tile = None
        # None is the fused skip it was
        assert torch.equal(on.forward_tiled(rect, ar, 32, base=None), on.forward_tiled(rect, ar, 32))
        assert torch.equal(on.forward_ensemble(x, a, "flip", base=None), on.forward_ensemble(x, a, "flip"))


def _step(m, x, a, g, base=None, ref=None):
    """one training step -> (sr, {name: grad}, d_base or None)"""
    m.zero_grad(set_to_none=True)
    b = None if base is None else base.clone().requires_grad_(True)
    kw = {} if b is None else {"base": b}
    if ref is not None:
        kw["ref"] = ref
    sr = m(x, a, **kw)
    assert sr.requires_grad
    (sr * g).sum().backward()
    return sr.detach(), {k: p.grad.clone() for k, p in m.named_parameters()}, None if b is None else b.grad.clone()


@pytest.mark.parametrize("prec,train_prec", [("fp32", None), ("bf16x3", None), ("bf16", "bf16"), ("fp32", "bf16x3"), ("bf16", None)])
def test_training_the_base_is_a_differentiable_add(prec, train_prec):
    """("bf16", None) is the lazy path: the bf16 inference kernels forward, an fp32 recompute in the backward"""
    import warnings
    x, a = _batch(21, 2, 4, 16)
    g = _rand((2, 1, 48, 48), 77)
    base = _rand((2, 48, 48), 6)
    off, on = _build(3, prec, train=True, train_precision=train_prec), _build(3, prec, True, train=True, train_precision=train_prec)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        sr0, g0, _ = _step(off, x, a, g)
        sr1, g1, d_base = _step(on, x, a, g, base)
        sr2, g2, d_base4 = _step(on, x, a, g, base.unsqueeze(1))
    assert torch.equal(sr1, sr0 + base.unsqueeze(1)) and torch.equal(sr2, sr1)
    assert set(g0) == set(g1) and all(torch.equal(g0[k], g1[k]) and torch.equal(g0[k], g2[k]) for k in g0)
    assert torch.equal(d_base, g[:, 0]) and torch.equal(d_base4, g)
    assert list(on.state_dict()) == list(off.state_dict())


def test_training_with_a_base_lrs_may_require_grad_and_frozen_parameters_still_give_d_base():
    x, a = _batch(23, 1, 3, 16)
    g = _rand((1, 1, 48, 48), 78)
    base = _rand((1, 48, 48), 7)
    off, on = _build(3, "fp32", train=True), _build(3, "fp32", True, train=True)
    xr, xo = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    (on(xr, a, base=base) * g).sum().backward()                  # the skip's own frame (the median, as data) is not in play: no error
    (off(xo, a) * g).sum().backward()
    assert torch.equal(xr.grad, xo.grad) and base.grad is None
    for p in on.parameters():
        p.requires_grad_(False)
    b = base.clone().requires_grad_(True)
    sr = on(x, a, base=b)
    sr.backward(g)
    assert torch.equal(b.grad, g[:, 0])
    with torch.no_grad():                                        # no graph: the inference kernels, the in-place add
        assert not on(x, a, base=b).requires_grad


def test_base_without_the_flag_and_bad_bases_raise():
    x, a = _batch(5, 2, 4, 32)
    base = _rand((2, 96, 96), 8)
    for flag in (None, False):
        off = _build(3, "fp32", flag)
        with torch.no_grad():
            for call in (lambda: off(x, a, base=base), lambda: off.forward_ensemble(x, a, "flip", base=base),
                         lambda: off.forward_tiled(x, a, 16, base=base)):
                with pytest.raises(ValueError, match="global_residual"):
                    call()
            plain = off(x, a)
            assert torch.equal(off(x, a, base=None), plain) and torch.equal(off.forward_tiled(x, a, 32, base=None), plain)
    on = _build(3, "fp32", True)
    with torch.no_grad():
        for bad, exc in ((base[:, :95], ValueError), (base[:1], ValueError), (base.unsqueeze(0), ValueError), (base.cpu(), TypeError),
                         (base.long(), TypeError), (base.cpu().numpy(), TypeError)):
            with pytest.raises(exc):
                on(x, a, base=bad)


def test_a_shift_and_add_frame_is_a_base():
    """the recipe of INTEGRATION.md: register_and_add -> HRNet(global_residual=True)(lrs, alphas, base=sr)"""
    x, a = _batch(41, 2, 5, 32)
    off, on = _build(3, "bf16"), _build(3, "bf16", True)
    with torch.no_grad():
        sr, weight, shifts = shiftadd.register_and_add(x, None, a, scale=3)
        assert tuple(sr.shape) == (2, 96, 96) and tuple(shifts.shape) == (2, 5, 2) and bool(torch.isfinite(sr).all())
        assert torch.equal(on(x, a, base=sr), off(x, a) + sr.unsqueeze(1))
