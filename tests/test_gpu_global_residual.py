"""GPU (-m gpu): HRNet's `global_residual` - every forward returns net(...) + up(frame), the frame being `ref` or the network's own
median - and the baseline table made with the same upsampler.

  off        key absent / None / False: forward, forward_ensemble, forward_tiled and a training step bit-identical to one another
  on         forward == upsample(frame, base=plain forward) bit for bit, in every precision and at every scale, with the median and with
             a composite frame; forward_ensemble and forward_tiled likewise (one add, after the mean / the last scatter); the tiled
             result of a square scene is the flagged whole-frame forward
  training   the parameter gradients are the unflagged model's bit for bit; a leaf `ref` receives the stem's d_ref plus up^T(g) within
             C T_bwd (tests/kernel_bounds.py, tests/upsample_ref.py) and one rounding of the sum; ref=None with lrs.requires_grad raises
  baseline   zeroed decode.final: the model IS upsample(frame); validate.baseline_table against the numpy oracle's shift_cPSNR of the
             clipped restatement at the relative 1e-4 of tests/test_gpu_ensemble.py, and a model that is the baseline scores 1.0
"""
import copy

import numpy as np
import pytest
import torch

import kernel_bounds as KB
import kt
import upsample_ref as R
import util
from hrnet_hip import composite, upsample
from oracle import hrnet_np as O
from oracle import synth, weights
from util import _state

pytestmark = pytest.mark.gpu

PRECS = ["fp32", "bf16", "bf16x3"]
ABSENT = object()


def _build(scale, prec, key=ABSENT, train=False, train_precision=None):
    from DeepNetworks.HRNet import HRNet
    cfg = copy.deepcopy(weights.HRNET_CONFIG)
    cfg["decoder"]["deconv"]["kernel_size"] = cfg["decoder"]["deconv"]["stride"] = scale
    if key is not ABSENT:
        cfg["global_residual"] = key
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


def _masks(shape, seed):
    return util.dev((np.random.Generator(np.random.PCG64(seed)).random(tuple(shape)) < 0.6).astype(np.float32))


def _cot(shape, seed=77):
    return util.dev(np.random.Generator(np.random.PCG64(seed)).standard_normal(tuple(shape)).astype(np.float32))


def _skip(frame, sr, scale):
    """what the flag adds, through the public function: sr (B,1,SH,SW) + up(frame (B,H,W))"""
    return upsample.upsample(frame, scale, base=sr[:, 0]).unsqueeze(1)


def _step(m, x, a, g, ref=None):
    """one training step -> (sr, {name: grad}, d_ref or None)"""
    m.zero_grad(set_to_none=True)
    r = None if ref is None else ref.clone().requires_grad_(True)
    sr = m(x, a) if r is None else m(x, a, ref=r)
    assert sr.requires_grad
    (sr * g).sum().backward()
    return sr.detach(), {k: p.grad.clone() for k, p in m.named_parameters()}, None if r is None else r.grad.clone()


# ----------------------------------------------------------------------------- off
def test_flag_off_changes_nothing():
    x, a = _batch(5, 2, 4, 32)
    rect = util.dev(synth.fast_batch(3, 1, 4, 48)[0][:, :, :, :40])
    ar = torch.ones(1, 4, device="cuda")
    g = _cot((2, 1, 96, 96))
    base = _build(3, "fp32")
    with torch.no_grad():
        want = (base(x, a), base.forward_ensemble(x, a, "flip"), base.forward_tiled(rect, ar, 32))
    want_step = _step(_build(3, "fp32", train=True), x, a, g)
    for key in (None, False):
        m = _build(3, "fp32", key)
        assert m.global_residual is key
        with torch.no_grad():
            got = (m(x, a), m.forward_ensemble(x, a, "flip"), m.forward_tiled(rect, ar, 32))
        assert all(torch.equal(p, q) for p, q in zip(got, want))
        sr, grads, _ = _step(_build(3, "fp32", key, train=True), x, a, g)
        assert torch.equal(sr, want_step[0]) and all(torch.equal(grads[k], want_step[1][k]) for k in grads)


# ----------------------------------------------------------------------------- on, inference
@pytest.mark.parametrize("scale", [2, 3, 4])
@pytest.mark.parametrize("prec", PRECS)
def test_forward_is_the_plain_forward_plus_the_upsampled_frame(prec, scale):
    x, a = _batch(5 + scale, 2, 4, 16)
    off, on = _build(scale, prec), _build(scale, prec, True)
    ref, filled = composite.masked_composite(x, _masks(x.shape, 8), a)
    with torch.no_grad():
        plain = off(x, a)
        got = on(x, a)
        assert got.dtype == torch.float32 and not got.requires_grad and tuple(got.shape) == tuple(plain.shape)
        assert torch.equal(got, _skip(_median(x), plain, scale)) and not torch.equal(got, plain)
        assert torch.equal(on(filled, a, ref=ref), _skip(ref, off(filled, a, ref=ref), scale))
        assert torch.equal(off(x, a), plain)                     # the in-place add touched the flagged model's own output only


@pytest.mark.parametrize("prec", PRECS)
def test_ensemble_adds_the_skip_once_after_the_mean(prec):
    x, a = _batch(63, 2, 4, 32)
    off, on = _build(3, prec), _build(3, prec, True)
    ref = composite.masked_composite(x, _masks(x.shape, 9), a)[0]
    with torch.no_grad():
        for mode in ("flip", "dihedral"):
            assert torch.equal(on.forward_ensemble(x, a, mode), _skip(_median(x), off.forward_ensemble(x, a, mode), 3))
        assert torch.equal(on.forward_ensemble(x, a, "flip", members_per_pass=3, ref=ref), _skip(ref, off.forward_ensemble(x, a, "flip", ref=ref), 3))
        on.ensemble = "flip"                                     # the attribute routes forward through the same sum: still one add
        assert torch.equal(on(x, a), on.forward_ensemble(x, a, "flip"))


@pytest.mark.parametrize("prec", PRECS)
def test_tiled_adds_the_skip_once_on_the_whole_scene(prec):
    off, on = _build(3, prec), _build(3, prec, True)
    rect = util.dev(synth.fast_batch(3, 2, 4, 48)[0][:, :, :, :40])             # (2, 4, 48, 40) in windows of 32: 2 x 2 of them
    ar = torch.ones(2, 4, device="cuda")
    ref = composite.masked_composite(rect, _masks(rect.shape, 4), ar)[0]
    with torch.no_grad():
        assert torch.equal(on.forward_tiled(rect, ar, 32), _skip(_median(rect), off.forward_tiled(rect, ar, 32), 3))
        assert torch.equal(on.forward_tiled(rect, ar, 32, windows_per_pass=1, ref=ref), _skip(ref, off.forward_tiled(rect, ar, 32, ref=ref), 3))
        assert torch.equal(on.forward_tiled(rect, ar, 32, ensemble="flip"), _skip(_median(rect), off.forward_tiled(rect, ar, 32, ensemble="flip"), 3))
        on.tile = 32
        assert torch.equal(on(rect, ar), on.forward_tiled(rect, ar, 32))
        on.tile = None
        x, a = _batch(304 + 56, 2, 4, 56)                        # a square scene: the flagged whole-frame forward
        whole = on(x, a)
        assert torch.equal(on.forward_tiled(x, a, 32), whole) and torch.equal(on.forward_tiled(x, a, 56), whole)
        assert torch.equal(on.forward_tiled(x, a, 32, ensemble="flip"), on.forward_ensemble(x, a, "flip"))


# ----------------------------------------------------------------------------- training
@pytest.mark.parametrize("prec,train_prec", [("fp32", None), ("bf16x3", None), ("bf16", "bf16"), ("fp32", "bf16x3"), ("bf16", None)])
def test_training_parameter_gradients_pass_through_unchanged(prec, train_prec):
    """("bf16", None) is the lazy path: the bf16 inference kernels forward, an fp32 recompute in the backward"""
    import warnings
    x, a = _batch(21, 2, 4, 16)
    g = _cot((2, 1, 48, 48))
    off, on = _build(3, prec, train=True, train_precision=train_prec), _build(3, prec, True, train=True, train_precision=train_prec)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        sr0, g0, _ = _step(off, x, a, g)
        sr1, g1, _ = _step(on, x, a, g)
    assert torch.equal(sr1, _skip(_median(x), sr0, 3))
    assert set(g0) == set(g1) and all(torch.equal(g0[k], g1[k]) for k in g0)
    assert list(on.state_dict()) == list(off.state_dict())


@pytest.mark.parametrize("prec", PRECS)
def test_training_a_leaf_ref_receives_the_stems_gradient_plus_the_adjoint(prec):
    x, a = _batch(22, 2, 5, 16)
    g = _cot((2, 1, 48, 48), 78)
    ref = composite.masked_composite(x, _masks(x.shape, 6), a, fill=False)[0]
    off, on = _build(3, prec, train=True, train_precision=prec), _build(3, prec, True, train=True, train_precision=prec)
    sr0, g0, d0 = _step(off, x, a, g, ref)
    sr1, g1, d1 = _step(on, x, a, g, ref)
    assert torch.equal(sr1, _skip(ref, sr0, 3)) and all(torch.equal(g0[k], g1[k]) for k in g0)
    gn = g[:, 0].cpu().numpy()
    want = d0.double().cpu().numpy() + R.adjoint(gn, 3)
    T = R.t_adjoint(gn, 3)
    bound = KB.C * T + 2.0 ** -24 * (np.abs(want) + KB.C * T)
    err = np.abs(d1.double().cpu().numpy() - want)
    print(f"{prec}: max |d_ref - (stem's d_ref + up^T g)| / bound = {float((err / bound).max()):.3e}")
    assert (err <= bound).all() and float(np.abs(R.adjoint(gn, 3)).max()) > 0
    # with every parameter frozen the frame alone asks for a gradient: the same d_ref
    for p in on.parameters():
        p.requires_grad_(False)
    r = ref.clone().requires_grad_(True)
    (on(x, a, ref=r) * g).sum().backward()
    assert torch.equal(r.grad, d1)


def test_training_ref_none_with_lrs_requiring_grad_raises():
    x, a = _batch(23, 1, 3, 16)
    on = _build(3, "fp32", True, train=True)
    with pytest.raises(NotImplementedError, match="ref="):
        on(x.clone().requires_grad_(True), a)
    xr = x.clone().requires_grad_(True)                          # with the frame given, lrs gets the network's own gradient and no more
    ref = _median(x)
    g = _cot((1, 1, 48, 48))
    (on(xr, a, ref=ref) * g).sum().backward()
    off = _build(3, "fp32", train=True)
    xo = x.clone().requires_grad_(True)
    (off(xo, a, ref=ref) * g).sum().backward()
    assert torch.equal(xr.grad, xo.grad)
    with torch.no_grad():                                        # no graph: nothing to lose, no error
        assert torch.equal(on(xr, a), _skip(ref, off(x, a), 3))


# ----------------------------------------------------------------------------- the baseline
def _zero_final(m):
    with torch.no_grad():
        m.decode.final.weight.zero_()
        m.decode.final.bias.zero_()
    return m


@pytest.mark.parametrize("prec", PRECS)
def test_zeroed_final_starts_at_the_bicubic_baseline(prec):
    x, a = _batch(31, 2, 4, 16)
    ref = composite.masked_composite(x, _masks(x.shape, 2), a, fill=False)[0]
    for scale in (2, 3, 4):
        on = _zero_final(_build(scale, prec, True))
        with torch.no_grad():
            assert bool((on(x, a) == upsample.upsample(_median(x), scale).unsqueeze(1)).all())
            assert bool((on(x, a, ref=ref) == upsample.upsample(ref, scale).unsqueeze(1)).all())
            assert bool((on(x, a) == upsample.baseline(x, scale=scale)).all())


def test_baseline_table_against_the_oracle_and_a_baseline_model_scores_one():
    from hrnet_hip import validate
    sets, want = [], {}
    for i in range(5):
        V = 3 + 2 * i                                            # 3 .. 11 views: below and above the nine the frame is made of
        lrs, alphas, hrs = synth.make_batch(50 + i, 1, V, 16, V)
        maps = (np.random.Generator(np.random.PCG64(i)).random((1, 48, 48)) > 0.1).astype(np.float32)
        name = f"imgset{i:04d}"
        sets.append((util.dev(lrs), util.dev(alphas), util.dev(hrs), util.dev(maps), [name]))
        n = min(V, 9)
        med = np.sort(lrs[0, :n].astype(np.float64), 0)[(n - 1) // 2]
        want[name] = O.shift_cpsnr(np.clip(R.forward(med, 3), 0, 1), hrs[0], maps[0])
    table = validate.baseline_table(sets)
    assert list(table) == list(want) and all(isinstance(v, float) for v in table.values())
    for k in want:
        print(f"{k}: baseline cPSNR {table[k]:.6f}, oracle {want[k]:.6f}")
        assert abs(table[k] - want[k]) <= 1e-4 * abs(want[k])
    # another cubic and border give another table; the scale comes from the shapes
    assert validate.baseline_table(sets, a=-0.5) != table and validate.baseline_table(sets, border_w=2) != table
    x2 = (sets[0][0], sets[0][1], sets[0][2][:, :32, :32].contiguous(), sets[0][3][:, :32, :32].contiguous(), ["x2"])
    w2 = O.shift_cpsnr(np.clip(R.forward(np.sort(x2[0][0].double().cpu().numpy(), 0)[1], 2), 0, 1), x2[2][0].cpu().numpy(), x2[3][0].cpu().numpy())
    assert abs(validate.baseline_table([x2])["x2"] - w2) <= 1e-4 * abs(w2)
    # the table is a baseline table: a model whose output is the baseline scores a normalised 1.0
    m = _zero_final(_build(3, "fp32", True))
    ev = validate.evaluate(m, sets, baseline_cpsnrs=table)
    assert ev.names == list(table) and abs(ev.score - 1.0) <= 1e-4
    assert np.all(np.abs(ev.cpsnr - np.array([want[k] for k in ev.names])) <= 1e-4 * np.abs(ev.cpsnr))
