"""GPU: the shift-searched loss (hrnet_hip.losses.shift_loss over hrn_shift_loss_train / hrn_shift_loss_backward)
against its fp64 restatement (tests/shift_loss_ref.py), against the kernels it generalises (hrn_shift_cpsnr, hrn_get_loss_train /
_backward), and as the tail of a training step without ShiftNet.

Shapes: B = 3 and (20, 20), (37, 53), (53, 37), (96, 96): one tile; odd, rectangular and no multiple of the 32 x 128 tile; the same
transposed (two tile rows); and a square with three tile rows; (280, 24) at border 8 and (1900, 12) at border 1 for the sum of a sample's
tiles (9 and 60 tiles in one column: a run longer than eight tiles, and runs that hold no tile).  Tolerances: 1e-5 relative on the reductions, as tests/test_gpu_losses.py
holds them; 1e-6 of the tensor's max-norm per element of d_srs (fp32 inputs taken exactly, three fp32 roundings per element - the
difference, the bias, the product with the coefficient - each <= 2^-24 relative, and fp64 statistics)."""
import itertools

import numpy as np
import pytest
import torch

import shift_loss_ref as R
import util

pytestmark = pytest.mark.gpu

SHAPES = [(20, 20), (37, 53), (53, 37), (96, 96)]
BORDERS = [0, 1, 3]
B = 3
TOL, GRAD_TOL = R.TOL, R.GRAD_TOL


def _random(H, W, seed, lo=0.0, hi=1.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    srs = (lo + (hi - lo) * rng.random((B, H, W))).astype(np.float32)
    hrs = rng.random((B, H, W), dtype=np.float32)
    maps = (rng.random((B, H, W)) > 0.1).astype(np.float32)
    return tuple(torch.from_numpy(x) for x in (srs, hrs, maps))


def _planted(H, W, border, seed):
    """srs iid uniform; the hrs window at the planted offset is the SR centre crop + N(0, 1e-3^2), the rest uniform.  One planted offset
    per sample: (0, 2 border), (border, border), (2 border, 0)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    srs = rng.random((B, H, W), dtype=np.float32)
    hrs = rng.random((B, H, W), dtype=np.float32)
    maps = (rng.random((B, H, W)) > 0.1).astype(np.float32)
    h, w = H - 2 * border, W - 2 * border
    plant = [(0, 2 * border), (border, border), (2 * border, 0)]
    for b, (u, v) in enumerate(plant):
        hrs[b, u:u + h, v:v + w] = srs[b, border:border + h, border:border + w] + 1e-3 * rng.standard_normal((h, w)).astype(np.float32)
    return tuple(torch.from_numpy(x) for x in (srs, hrs, maps)), plant


_cache = {}


def _ref(key, make):
    """one restatement (and its fp64 autograd gradient) per input set, shared by the tests that need it"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _restated(srs, hrs, maps, metric, border, clip, d_out=None):
    s = srs.double().requires_grad_(True)
    out, k, cm = R.shift_loss(s, hrs, maps, metric, border, clip)
    (out * (1.0 if d_out is None else d_out.double())).sum().backward()
    return out.detach(), k, cm, s.grad


def _cuda(*ts):
    return tuple(t.cuda() for t in ts)


# ----------------------------------------------------------------------------- forward
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_is_the_restatement(shape):
    from hrnet_hip import losses
    H, W = shape
    for border, clip in itertools.product(BORDERS, (False, True)):
        lo, hi = (-0.2, 1.2) if clip else (0.0, 1.0)
        x = _random(H, W, 11 + border, lo, hi)
        d = _cuda(*x)
        for metric in ("cMSE", "cPSNR"):
            want, k, _, _ = _ref(("rand", shape, border, clip, metric), lambda: _restated(*x, metric, border, clip))
            got, shift = losses.shift_loss(*d, metric=metric, border_w=border, clip=clip, return_shift=True)
            assert got.dtype == torch.float32 and tuple(got.shape) == (B,) and shift.dtype == torch.int64 and tuple(shift.shape) == (B, 2)
            e = util.rel_err(got.cpu().numpy(), want.numpy())
            print(f"forward {shape} border {border} clip {clip} {metric}: rel err {e:.2e}")
            assert e <= TOL, (shape, border, clip, metric, e)


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] == s[1]])
def test_forward_is_shift_cpsnr_on_squares(shape):
    from hrnet_hip import binding, losses
    for border in BORDERS:
        d = _cuda(*_random(*shape, 21 + border, -0.2, 1.2))
        want = binding.shift_cpsnr(*d, border_w=border, clip=False)
        got = losses.shift_loss(*d, metric="cPSNR", border_w=border, clip=False)
        assert util.rel_err(got.cpu().numpy(), want.cpu().numpy()) <= TOL


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] == s[1]])
def test_without_border_it_is_get_loss(shape):
    """beta = 0: forward and backward are hrn_get_loss_train / hrn_get_loss_backward with crop = 0"""
    from hrnet_hip import binding
    d = _cuda(*_random(*shape, 31))
    d_out = torch.tensor([1.0, -0.5, 2.0], device="cuda")
    for metric in ("cMSE", "cPSNR"):
        want, wstats = binding.get_loss_train(*d, metric, 0)
        got, stats = binding.shift_loss_train(*d, metric, 0, False)
        assert util.rel_err(got.cpu().numpy(), want.cpu().numpy()) <= TOL
        assert util.rel_err(stats[:, :3].cpu().numpy(), wstats[:, :3].cpu().numpy()) <= TOL and (stats[:, 3] == 0).all()
        wgrad = binding.get_loss_backward(*d, wstats, d_out, metric, 0)
        grad = binding.shift_loss_backward(*d, stats, d_out, metric, 0, False)
        assert util.rel_err(grad.cpu().numpy(), wgrad.cpu().numpy()) <= TOL


def test_rectangular_input_reaches_the_c_abi_as_given():
    """(B,1,H,W) srs is srs[:, 0]; a non-contiguous view is used by value"""
    from hrnet_hip import losses
    s, h, m = _cuda(*_random(37, 53, 41))
    want = losses.shift_loss(s, h, m)
    assert torch.equal(losses.shift_loss(s[:, None], h, m), want)
    st = s.transpose(1, 2).contiguous().transpose(1, 2)
    assert not st.is_contiguous() and torch.equal(losses.shift_loss(st, h, m), want)


# ----------------------------------------------------------------------------- the selected offset
@pytest.mark.parametrize("shape", SHAPES)
def test_selected_offset_is_the_planted_one(shape):
    from hrnet_hip import binding, losses
    H, W = shape
    compared = 0
    for border in BORDERS:
        x, plant = _planted(H, W, border, 51 + border)
        _, k, cm, _ = _ref(("plant", shape, border), lambda: _restated(*x, "cPSNR", border, False))
        nb = 2 * border + 1
        assert k.tolist() == [u * nb + v for u, v in plant]
        if nb > 1:      # the runner-up is far below: > 50 dB, so no sample is near a tie
            assert float((10 * torch.log10(torch.sort(cm, 1).values[:, 1] / torch.sort(cm, 1).values[:, 0])).min()) > 50.0
        got, shift = losses.shift_loss(*_cuda(*x), border_w=border, return_shift=True)
        stats = binding.shift_loss_train(*_cuda(*x), "cPSNR", border, False)[1]
        assert stats[:, 3].long().cpu().tolist() == k.tolist()
        assert torch.equal(shift.cpu(), R.offsets(k, border))
        compared += B
    assert compared == B * len(BORDERS)          # none excluded


# ----------------------------------------------------------------------------- backward
def _check_grad(got, want, border, what):
    got, want = got.cpu().double(), want
    scale = float(want.abs().amax())
    e = float((got - want).abs().amax()) / scale
    print(f"d_srs {what}: max err / max-norm {e:.2e}")
    assert e <= GRAD_TOL, (what, e)
    if border:
        frame = torch.ones_like(got, dtype=torch.bool)
        frame[:, border:-border, border:-border] = False
        assert (got[frame] == 0).all(), what


@pytest.mark.parametrize("shape", SHAPES)
def test_gradient_is_fp64_autograd(shape):
    from hrnet_hip import losses
    H, W = shape
    d_out = torch.tensor([1.0, -0.5, 2.0])
    dropped, total = 0, 0
    for border, metric in itertools.product(BORDERS, ("cMSE", "cPSNR")):
        # planted inputs: every sample compared
        x, _ = _planted(H, W, border, 51 + border)
        _, _, _, want = _ref(("plantgrad", shape, border, metric), lambda: _restated(*x, metric, border, False, d_out))
        s = x[0].cuda().requires_grad_(True)
        (losses.shift_loss(s, x[1].cuda(), x[2].cuda(), metric=metric, border_w=border) * d_out.cuda()).sum().backward()
        for b in range(B):
            _check_grad(s.grad[b:b + 1], want[b:b + 1], border, f"planted {shape} border {border} {metric} sample {b}")
        # random inputs: a sample whose two lowest cMSE are within 1e-6 relative could select either offset
        x = _random(H, W, 11 + border)
        _, _, cm, want = _ref(("randgrad", shape, border, metric), lambda: _restated(*x, metric, border, False, d_out))
        keep = R.top_two_gap(cm) > 1e-6
        dropped += int((~keep).sum())
        total += B
        s = x[0].cuda().requires_grad_(True)
        (losses.shift_loss(s, x[1].cuda(), x[2].cuda(), metric=metric, border_w=border) * d_out.cuda()).sum().backward()
        for b in range(B):
            if keep[b]:
                _check_grad(s.grad[b:b + 1], want[b:b + 1], border, f"random {shape} border {border} {metric} sample {b}")
    assert dropped == 0 and total == B * len(BORDERS) * 2


@pytest.mark.parametrize("shape", SHAPES)
def test_clipped_gradient_is_zero_exactly_where_clamped(shape):
    from hrnet_hip import losses
    H, W = shape
    for border in BORDERS:
        x = _random(H, W, 61 + border, -0.2, 1.2)
        _, _, cm, want = _ref(("clipgrad", shape, border), lambda: _restated(*x, "cPSNR", border, True))
        assert float(R.top_two_gap(cm).min()) > 1e-6
        s = x[0].cuda().requires_grad_(True)
        losses.shift_loss(s, x[1].cuda(), x[2].cuda(), border_w=border, clip=True).sum().backward()
        _check_grad(s.grad, want, border, f"clipped {shape} border {border}")
        clamped = (x[0] < 0) | (x[0] > 1)
        assert clamped.any() and (s.grad.cpu()[clamped] == 0).all()
        inner = torch.zeros_like(clamped)
        inner[:, border:H - border, border:W - border] = True
        live = inner & ~clamped & (want != 0)
        assert (s.grad.cpu()[live] != 0).all()


def test_d_out_scales_the_gradient():
    from hrnet_hip import binding
    d = _cuda(*_random(37, 53, 71))
    _, stats = binding.shift_loss_train(*d, "cPSNR", 3, False)
    one = binding.shift_loss_backward(*d, stats, torch.ones(B, device="cuda"), "cPSNR", 3, False)
    d_out = torch.tensor([2.0, -0.25, 0.0], device="cuda")              # powers of two: the scaling is exact
    got = binding.shift_loss_backward(*d, stats, d_out, "cPSNR", 3, False)
    assert torch.equal(got, one * d_out[:, None, None]) and (got[2] == 0).all() and (one[2] != 0).any()


def test_no_clear_pixel_gives_nan_and_a_zero_gradient():
    from hrnet_hip import losses
    s, h, m = _random(37, 53, 81)
    m[1] = 0
    s = s.cuda().requires_grad_(True)
    out, shift = losses.shift_loss(s, h.cuda(), m.cuda(), return_shift=True)
    assert torch.isnan(out[1]) and torch.isfinite(out[[0, 2]]).all()
    out[[0, 1, 2]].sum().backward()
    assert (s.grad[1] == 0).all() and torch.isfinite(s.grad).all() and (s.grad[0] != 0).any()


def test_two_runs_are_bit_identical():
    from hrnet_hip import binding
    d = _cuda(*_random(96, 96, 91))
    d_out = torch.tensor([1.0, -0.5, 2.0], device="cuda")
    runs = []
    for _ in range(2):
        out, stats = binding.shift_loss_train(*d, "cPSNR", 3, False)
        runs.append((out, stats, binding.shift_loss_backward(*d, stats, d_out, "cPSNR", 3, False)))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_large_border_and_wide_frames():
    """border 8 (the widest LDS halo) and a frame wider than one 128-pixel tile column, against the restatement"""
    from hrnet_hip import losses
    rng = np.random.Generator(np.random.PCG64(95))
    for (H, W), border in (((40, 300), 8), ((70, 139), 5)):
        x = tuple(torch.from_numpy(a) for a in (rng.random((2, H, W), dtype=np.float32), rng.random((2, H, W), dtype=np.float32),
                                                (rng.random((2, H, W)) > 0.1).astype(np.float32)))
        want, k, _ = R.shift_loss(*x, "cPSNR", border)
        got, shift = losses.shift_loss(*_cuda(*x), border_w=border, return_shift=True)
        assert util.rel_err(got.cpu().numpy(), want.numpy()) <= TOL and torch.equal(shift.cpu(), R.offsets(k, border))


def test_long_columns_of_tiles():
    """9 tiles added as one run (a block of eight and a tail of one) and 60 tiles added in 37 runs of 2, the last 7 of them empty:
    forward, selected offset and gradient against the restatement, no sample excluded"""
    from hrnet_hip import losses
    d_out = torch.tensor([1.0, -0.5, 2.0])
    for (H, W), border in (((280, 24), 8), ((1900, 12), 1)):
        x = _random(H, W, 11 + border)
        d = _cuda(*x)
        for metric in ("cMSE", "cPSNR"):
            want, k, cm, wgrad = _ref(("tall", (H, W), border, metric), lambda: _restated(*x, metric, border, False, d_out))
            assert float(R.top_two_gap(cm).min()) > 1e-6
            s = d[0].clone().requires_grad_(True)
            got, shift = losses.shift_loss(s, d[1], d[2], metric=metric, border_w=border, return_shift=True)
            (got * d_out.cuda()).sum().backward()
            e = util.rel_err(got.detach().cpu().numpy(), want.numpy())
            print(f"forward ({H}, {W}) border {border} {metric}: rel err {e:.2e}")
            assert e <= TOL and torch.equal(shift.cpu(), R.offsets(k, border))
            _check_grad(s.grad, wgrad, border, f"tall ({H}, {W}) border {border} {metric}")


def test_a_sample_does_not_depend_on_its_batch():
    from hrnet_hip import binding
    d = _cuda(*_random(96, 96, 141))
    d_out = torch.tensor([1.0, -0.5, 2.0], device="cuda")
    for metric in ("cMSE", "cPSNR"):
        out, stats = binding.shift_loss_train(*d, metric, 3, True)
        grad = binding.shift_loss_backward(*d, stats, d_out, metric, 3, True)
        for b in range(B):
            one = tuple(t[b:b + 1].contiguous() for t in d)
            out1, stats1 = binding.shift_loss_train(*one, metric, 3, True)
            grad1 = binding.shift_loss_backward(*one, stats1, d_out[b:b + 1], metric, 3, True)
            assert torch.equal(out1, out[b:b + 1]) and torch.equal(stats1, stats[b:b + 1]) and torch.equal(grad1, grad[b:b + 1])


# ----------------------------------------------------------------------------- dispatcher
def test_opcheck():
    ops = torch.ops.hrnet_hip
    assert hasattr(ops, "shift_loss_train") and hasattr(ops, "shift_loss_backward")
    s, h, m = _cuda(*_random(37, 53, 101))
    checks = ("test_schema", "test_faketensor", "test_autograd_registration")
    for args in ((s, h, m, "cPSNR", 3, False), (s.clone().requires_grad_(True), h, m, "cMSE", 1, True)):
        torch.library.opcheck(ops.shift_loss_train.default, args, test_utils=checks)
    _, stats = ops.shift_loss_train(s, h, m, "cPSNR", 3, False)
    torch.library.opcheck(ops.shift_loss_backward.default, (s, h, m, stats, torch.ones(B, device="cuda"), "cPSNR", 3, False), test_utils=checks)


# ----------------------------------------------------------------------------- behind HRNet
def _batch(Bn, V, S, scale, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    lrs = rng.random((Bn, V, S, S), dtype=np.float32)
    alphas = np.ones((Bn, V), np.float32)
    hrs = rng.random((Bn, scale * S, scale * S), dtype=np.float32)
    maps = (rng.random((Bn, scale * S, scale * S)) > 0.1).astype(np.float32)
    return tuple(util.dev(a) for a in (lrs, alphas, hrs, maps))


def test_chain_through_hrnet_at_a_size_shiftnet_cannot_train():
    """48 x 48 SR (below ShiftNet's 128-pixel window): the parameter gradients of the loss are the model's backward of d_srs"""
    from hrnet_hip import binding, losses
    model = util._fresh_model(precision="fp32")
    lrs, alphas, hrs, maps = _batch(2, 4, 16, 3, 111)
    params = list(model.parameters())
    srs = model(lrs, alphas)
    assert tuple(srs.shape) == (2, 1, 48, 48)
    (-losses.shift_loss(srs, hrs, maps)).mean().backward()
    got = [p.grad.clone() for p in params]
    srs2 = model(lrs, alphas)
    assert torch.equal(srs2, srs)
    _, stats = binding.shift_loss_train(srs2.detach()[:, 0], hrs, maps, "cPSNR", 3, False)
    d_srs = binding.shift_loss_backward(srs2.detach()[:, 0], hrs, maps, stats, torch.full((2,), -0.5, device="cuda"), "cPSNR", 3, False)
    want = torch.autograd.grad(srs2, params, grad_outputs=d_srs[:, None])
    assert any(float(g.abs().max()) > 0 for g in got)
    for g, w in zip(got, want):
        assert torch.equal(g, w)


def test_five_bf16_steps_without_shiftnet(monkeypatch):
    """Plumbing only (no claim about accuracy), in the pattern of test_five_bf16_steps_from_an_augmented_cache: HRNet in bf16 training
    precision, the searched loss and FusedAdam over HRNet's parameters alone; no ShiftNet is ever constructed."""
    import DeepNetworks.ShiftNet as SN
    from DeepNetworks.HRNet import HRNet
    from hrnet_hip import losses
    from hrnet_hip.optim import FusedAdam
    from oracle import weights

    built = []
    monkeypatch.setattr(SN.ShiftNet, "__init__", lambda self, *a, **k: built.append(1))
    fusion = HRNet(weights.HRNET_CONFIG)
    fusion.load_state_dict(weights.to_torch_state(weights.hrnet_state(1234)))
    fusion.train_precision = "bf16"
    fusion = fusion.cuda().train()
    before = [p.detach().clone() for p in fusion.parameters()]
    optimizer = FusedAdam(list(fusion.parameters()), lr=1e-4)
    lrs, alphas, hrs, maps = _batch(2, 4, 16, 3, 121)
    seen = []
    for _ in range(5):
        optimizer.zero_grad()
        loss = (-losses.shift_loss(fusion(lrs, alphas), hrs, maps)).mean()
        loss.backward()
        optimizer.step()
        seen.append(float(loss))
    assert np.isfinite(seen).all() and not built
    assert sum(p.numel() for g in optimizer.param_groups for p in g["params"]) == sum(p.numel() for p in fusion.parameters())
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, fusion.parameters()))


# ----------------------------------------------------------------------------- rectangular scoring
def test_evaluate_scores_a_rectangular_scene_and_leaves_square_scores_alone():
    from hrnet_hip import binding, validate
    m = util.hip_hrnet("fp32")
    rng = np.random.Generator(np.random.PCG64(131))
    sets, want = [], []
    for i in range(2):
        lrs = util.dev(rng.random((2, 3, 40, 72), dtype=np.float32))
        alphas = util.dev(np.ones((2, 3), np.float32))
        hrs = util.dev(rng.random((2, 120, 216), dtype=np.float32))
        maps = util.dev((rng.random((2, 120, 216)) > 0.1).astype(np.float32))
        sets.append((lrs, alphas, hrs, maps, [f"imgset{2 * i + j:04d}" for j in range(2)]))
        with torch.no_grad():
            srs = m.forward_tiled(lrs, alphas, 32)[:, 0]
        want.append(R.shift_loss(srs.cpu(), hrs.cpu(), maps.cpu(), "cPSNR", 3, clip=True)[0].numpy())
    ev = validate.evaluate(m, sets, tile=32)
    assert ev.names == [f"imgset{i:04d}" for i in range(4)]
    assert util.rel_err(ev.cpsnr, np.concatenate(want)) <= TOL
    assert abs(ev.score + np.concatenate(want).mean()) <= TOL * abs(ev.score)
    # a square scene keeps hrn_shift_cpsnr, bit for bit
    lrs = util.dev(rng.random((2, 3, 32, 32), dtype=np.float32))
    alphas = util.dev(np.ones((2, 3), np.float32))
    hrs = util.dev(rng.random((2, 96, 96), dtype=np.float32))
    maps = util.dev((rng.random((2, 96, 96)) > 0.1).astype(np.float32))
    with torch.no_grad():
        srs = m(lrs, alphas)[:, 0]
    ev = validate.evaluate(m, [(lrs, alphas, hrs, maps)])
    assert np.array_equal(ev.cpsnr, binding.shift_cpsnr(srs, hrs, maps, 3, True).double().cpu().numpy())
