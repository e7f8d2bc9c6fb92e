"""GPU: the shift-searched L1 / Charbonnier loss (hrnet_hip.losses.cl1_loss over hrn_cl1_loss_train / hrn_cl1_loss_backward, DESIGN.md
section 7m) against its fp64 restatement (tests/cl1_ref.py), and as the tail of a training step without ShiftNet.

Shapes: B = 3 and (20, 20), (37, 53), (53, 37), (96, 96) - one tile; odd, rectangular and no multiple of the 32 x 128 tile; the same
transposed (two tile rows); three tile rows - at borders 0, 1, 3, plus (40, 300) at border 8 and (70, 139) at border 5 (the widest
halo, more than one tile column) and (280, 24) at border 8 and (1900, 12) at border 1 (9 and 60 tiles in one column: the sum of a
sample's tiles in runs longer than eight tiles, and with runs that hold no tile), each at eps = 0 (L1) and 1e-3 (Charbonnier).  Tolerances, as tests/test_gpu_shift_loss.py holds
them: 1e-5 relative on out, n, bias, cL1 and sigma (fp64 sums of exact fp32 inputs; out is one fp32 rounding of cL1); 1e-6 of the
tensor's max-norm per element of d_srs (e, rho' and the product in fp64, one fp32 rounding of the result, <= 2^-24 relative); k* and
the returned shifts exact.  No sample is excluded: tests/test_cl1_host.py asserts on the CPU that no input set of tests/cl1_cases.py
is near a tie of its two best offsets or has an |e| near a sign flip."""
import numpy as np
import pytest
import torch

import cl1_cases as C
import cl1_ref as R
import util

pytestmark = pytest.mark.gpu

B = C.B
TOL, GRAD_TOL = C.TOL, C.GRAD_TOL
D_OUT = torch.tensor([1.0, -0.5, 2.0])

_cache = {}


def _restated(kind, shape, border, eps):
    """one restatement (and its fp64 autograd gradient under D_OUT) per input set and eps, shared by the tests that need it:
    -> (inputs, clip, out, k, stats, d_srs)"""
    key = (kind, shape, border, eps)
    if key not in _cache:
        x, clip = C.case(kind, shape, border)
        s = x[0].double().requires_grad_(True)
        out, k, _, stats = R.cl1_loss(s, x[1], x[2], border, clip, eps)
        (out * D_OUT.double()).sum().backward()
        _cache[key] = (x, clip, out.detach(), k, stats, s.grad)
    return _cache[key]


def _cuda(*ts):
    return tuple(t.cuda() for t in ts)


def _check_forward(kind, shape, border, eps):
    from hrnet_hip import binding, losses
    x, clip, want, k, wstats, _ = _restated(kind, shape, border, eps)
    d = _cuda(*x)
    got, shift = losses.cl1_loss(*d, border_w=border, clip=clip, eps=eps, return_shift=True)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B,) and shift.dtype == torch.int64 and tuple(shift.shape) == (B, 2)
    out, stats = binding.cl1_loss_train(*d, border, clip, eps)
    assert torch.equal(out, got) and stats.dtype == torch.float64 and tuple(stats.shape) == (B, 5)
    stats = stats.cpu()
    e_out = util.rel_err(got.cpu().numpy(), want.numpy())
    e_stats = max(util.rel_err(stats[:, j].numpy(), wstats[:, j].numpy()) for j in (0, 1, 2, 4))
    print(f"forward {kind} {shape} border {border} clip {clip} eps {eps}: out {e_out:.2e}, n / bias / cL1 / sigma {e_stats:.2e}")
    assert stats[:, 3].long().tolist() == k.tolist() and torch.equal(shift.cpu(), R.offsets(k, border))
    assert e_out <= TOL and e_stats <= TOL, (kind, shape, border, eps, e_out, e_stats)
    return k


def _check_grad(got, want, border, what):
    got = got.cpu().double()
    e = float((got - want).abs().amax()) / float(want.abs().amax())
    print(f"d_srs {what}: max err / max-norm {e:.2e}")
    assert e <= GRAD_TOL, (what, e)
    if border:
        frame = torch.ones_like(got, dtype=torch.bool)
        frame[:, border:-border, border:-border] = False
        assert (got[frame] == 0).all(), what


def _device_grad(x, border, clip, eps, d_out=D_OUT):
    from hrnet_hip import losses
    s = x[0].cuda().requires_grad_(True)
    (losses.cl1_loss(s, x[1].cuda(), x[2].cuda(), border_w=border, clip=clip, eps=eps) * d_out.cuda()).sum().backward()
    return s.grad


# ----------------------------------------------------------------------------- forward
@pytest.mark.parametrize("eps", C.EPS)
@pytest.mark.parametrize("shape", C.SHAPES)
def test_forward_is_the_restatement(shape, eps):
    compared = 0
    for border in C.BORDERS:
        for kind in ("rand", "clip"):            # clip off on [0, 1), clip on on (-0.2, 1.2)
            _check_forward(kind, shape, border, eps)
            compared += B
    assert compared == B * len(C.BORDERS) * 2    # none excluded


@pytest.mark.parametrize("eps", C.EPS)
@pytest.mark.parametrize("shape", C.SHAPES)
def test_selected_offset_is_the_planted_one(shape, eps):
    for border in C.BORDERS:
        plant = C.planted(*shape, border, 51 + border)[1]
        nb = 2 * border + 1
        assert _check_forward("plant", shape, border, eps).tolist() == [u * nb + v for u, v in plant]


@pytest.mark.parametrize("eps", C.EPS)
def test_large_border_and_wide_frames(eps):
    """border 8 (the widest LDS halo) and frames wider than one 128-pixel tile column: forward and gradient"""
    for shape, border in C.WIDE:
        x, clip, _, _, _, want = _restated("wide", shape, border, eps)
        _check_forward("wide", shape, border, eps)
        _check_grad(_device_grad(x, border, clip, eps), want, border, f"wide {shape} border {border} eps {eps}")


@pytest.mark.parametrize("eps", C.EPS)
def test_long_columns_of_tiles(eps):
    """9 tiles added as one run (a block of eight and a tail of one) and 60 tiles added in 56 runs of 2, the last 26 of them empty:
    forward, selected offset and gradient"""
    for shape, border in C.TALL:
        x, clip, _, _, _, want = _restated("rand", shape, border, eps)
        _check_forward("rand", shape, border, eps)
        _check_grad(_device_grad(x, border, clip, eps), want, border, f"tall {shape} border {border} eps {eps}")


@pytest.mark.parametrize("eps", C.EPS)
def test_the_map_is_a_weight(eps):
    """maps in {0, 0.5, 1}: a binarised map gives another n, bias, value and gradient"""
    for shape, border in (((37, 53), 3), ((96, 96), 1)):
        x, clip, _, _, wstats, want = _restated("weight", shape, border, eps)
        binarised = R.cl1_loss(x[0], x[1], (x[2] != 0).float(), border, clip, eps)[3]
        assert ((x[2] == 0.5).sum((1, 2)) > 0).all() and (util.rel_err(binarised[:, :3].numpy(), wstats[:, :3].numpy()) > 100 * TOL)
        _check_forward("weight", shape, border, eps)
        _check_grad(_device_grad(x, border, clip, eps), want, border, f"weighted {shape} border {border} eps {eps}")


def test_input_reaches_the_c_abi_as_given():
    """(B,1,H,W) srs is srs[:, 0]; a non-contiguous view is used by value; with and without a graph the same bits"""
    from hrnet_hip import losses
    s, h, m = _cuda(*C.random(37, 53, 41))
    for eps in C.EPS:
        want = losses.cl1_loss(s, h, m, eps=eps)
        assert torch.equal(losses.cl1_loss(s[:, None], h, m, eps=eps), want)
        st = s.transpose(1, 2).contiguous().transpose(1, 2)
        assert not st.is_contiguous() and torch.equal(losses.cl1_loss(st, h, m, eps=eps), want)
        with_graph = losses.cl1_loss(s.clone().requires_grad_(True), h, m, eps=eps)
        assert with_graph.requires_grad and not want.requires_grad and torch.equal(with_graph.detach(), want)


# ----------------------------------------------------------------------------- backward
@pytest.mark.parametrize("eps", C.EPS)
@pytest.mark.parametrize("shape", C.SHAPES)
def test_gradient_is_fp64_autograd(shape, eps):
    compared = 0
    for border in C.BORDERS:
        for kind in ("plant", "rand"):
            x, clip, _, _, _, want = _restated(kind, shape, border, eps)
            grad = _device_grad(x, border, clip, eps)
            for b in range(B):
                _check_grad(grad[b:b + 1], want[b:b + 1], border, f"{kind} {shape} border {border} eps {eps} sample {b}")
                compared += 1
    assert compared == B * len(C.BORDERS) * 2    # none excluded


@pytest.mark.parametrize("eps", C.EPS)
@pytest.mark.parametrize("shape", C.SHAPES)
def test_clipped_gradient_is_zero_exactly_where_clamped(shape, eps):
    H, W = shape
    for border in C.BORDERS:
        x, clip, _, _, _, want = _restated("clip", shape, border, eps)
        assert clip
        grad = _device_grad(x, border, True, eps)
        _check_grad(grad, want, border, f"clipped {shape} border {border} eps {eps}")
        clamped = (x[0] < 0) | (x[0] > 1)
        assert clamped.any() and (grad.cpu()[clamped] == 0).all()
        inner = torch.zeros_like(clamped)
        inner[:, border:H - border, border:W - border] = True
        live = inner & ~clamped & (want != 0)
        assert live.any() and (grad.cpu()[live] != 0).all()


def test_d_out_scales_the_gradient():
    from hrnet_hip import binding
    d = _cuda(*C.random(37, 53, 71))
    for eps in C.EPS:
        _, stats = binding.cl1_loss_train(*d, 3, False, eps)
        one = binding.cl1_loss_backward(*d, stats, torch.ones(B, device="cuda"), 3, False, eps)
        d_out = torch.tensor([2.0, -0.25, 0.0], device="cuda")              # powers of two: the scaling is exact
        got = binding.cl1_loss_backward(*d, stats, d_out, 3, False, eps)
        assert torch.equal(got, one * d_out[:, None, None]) and (got[2] == 0).all() and (one[2] != 0).any()


def test_no_clear_pixel_gives_nan_and_a_zero_gradient():
    from hrnet_hip import binding, losses
    s, h, m = C.random(37, 53, 81)
    m[1] = 0
    for eps in C.EPS:
        sd = s.cuda().requires_grad_(True)
        out, shift = losses.cl1_loss(sd, h.cuda(), m.cuda(), eps=eps, return_shift=True)
        assert torch.isnan(out[1]) and torch.isfinite(out[[0, 2]]).all() and shift[1, 0] == -4                # the (-border_w - 1, ...) row
        out.sum().backward()
        assert (sd.grad[1] == 0).all() and torch.isfinite(sd.grad).all() and (sd.grad[0] != 0).any() and (sd.grad[2] != 0).any()
        stats = binding.cl1_loss_train(s.cuda(), h.cuda(), m.cuda(), 3, False, eps)[1].cpu()
        assert stats[1, [0, 1, 3, 4]].tolist() == [0.0, 0.0, -1.0, 0.0] and torch.isnan(stats[1, 2])
        # the neighbours are untouched: their slices of a batch without the empty sample, bit for bit
        keep = [0, 2]
        sk = s[keep].cuda().requires_grad_(True)
        outk = losses.cl1_loss(sk, h[keep].cuda(), m[keep].cuda(), eps=eps)
        outk.sum().backward()
        assert torch.equal(outk, out[keep]) and torch.equal(sk.grad, sd.grad[keep])


def test_two_runs_are_bit_identical():
    from hrnet_hip import binding
    d = _cuda(*C.random(96, 96, 91))
    d_out = D_OUT.cuda()
    for eps in C.EPS:
        runs = []
        for _ in range(2):
            out, stats = binding.cl1_loss_train(*d, 3, False, eps)
            runs.append((out, stats, binding.cl1_loss_backward(*d, stats, d_out, 3, False, eps)))
        for a, b in zip(*runs):
            assert torch.equal(a, b) and not torch.isnan(a).any()


@pytest.mark.parametrize("eps", C.EPS)
def test_a_sample_does_not_depend_on_its_batch(eps):
    from hrnet_hip import binding
    for shape, border in (((96, 96), 3), ((70, 139), 5)):
        d = _cuda(*C.random(*shape, 141))
        d_out = D_OUT.cuda()
        out, stats = binding.cl1_loss_train(*d, border, True, eps)
        grad = binding.cl1_loss_backward(*d, stats, d_out, border, True, eps)
        for b in range(B):
            one = tuple(t[b:b + 1].contiguous() for t in d)
            out1, stats1 = binding.cl1_loss_train(*one, border, True, eps)
            grad1 = binding.cl1_loss_backward(*one, stats1, d_out[b:b + 1], border, True, eps)
            assert torch.equal(out1, out[b:b + 1]) and torch.equal(stats1, stats[b:b + 1]) and torch.equal(grad1, grad[b:b + 1])


# ----------------------------------------------------------------------------- dispatcher
def test_opcheck():
    ops = torch.ops.hrnet_hip
    assert hasattr(ops, "cl1_loss_train") and hasattr(ops, "cl1_loss_backward")
    s, h, m = _cuda(*C.random(37, 53, 101))
    checks = ("test_schema", "test_faketensor", "test_autograd_registration")
    for args in ((s, h, m, 3, False, 0.0), (s.clone().requires_grad_(True), h, m, 1, True, 1e-3)):
        torch.library.opcheck(ops.cl1_loss_train.default, args, test_utils=checks)
    _, stats = ops.cl1_loss_train(s, h, m, 3, False, 0.0)
    torch.library.opcheck(ops.cl1_loss_backward.default, (s, h, m, stats, torch.ones(B, device="cuda"), 3, False, 0.0), test_utils=checks)


# ----------------------------------------------------------------------------- behind HRNet
def _batch(Bn, V, S, scale, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    lrs = rng.random((Bn, V, S, S), dtype=np.float32)
    alphas = np.ones((Bn, V), np.float32)
    hrs = rng.random((Bn, scale * S, scale * S), dtype=np.float32)
    maps = (rng.random((Bn, scale * S, scale * S)) > 0.1).astype(np.float32)
    return tuple(util.dev(a) for a in (lrs, alphas, hrs, maps))


@pytest.mark.parametrize("eps", C.EPS)
def test_chain_through_hrnet_at_a_size_shiftnet_cannot_train(eps):
    """48 x 48 SR (below ShiftNet's 128-pixel window): the parameter gradients of the loss are the model's backward of d_srs"""
    from hrnet_hip import binding, losses
    model = util._fresh_model(precision="fp32")
    lrs, alphas, hrs, maps = _batch(2, 4, 16, 3, 111)
    params = list(model.parameters())
    srs = model(lrs, alphas)
    assert tuple(srs.shape) == (2, 1, 48, 48)
    losses.cl1_loss(srs, hrs, maps, eps=eps).mean().backward()
    got = [p.grad.clone() for p in params]
    srs2 = model(lrs, alphas)
    assert torch.equal(srs2, srs)
    _, stats = binding.cl1_loss_train(srs2.detach()[:, 0], hrs, maps, 3, False, eps)
    d_srs = binding.cl1_loss_backward(srs2.detach()[:, 0], hrs, maps, stats, torch.full((2,), 0.5, device="cuda"), 3, False, eps)
    want = torch.autograd.grad(srs2, params, grad_outputs=d_srs[:, None])
    assert any(float(g.abs().max()) > 0 for g in got)
    for g, w in zip(got, want):
        assert torch.equal(g, w)


def test_five_bf16_steps_without_shiftnet(monkeypatch):
    """Plumbing only (no claim about accuracy): HRNet in bf16 training precision, the searched L1 and FusedAdam over HRNet's parameters
    alone; no ShiftNet is ever constructed."""
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
        loss = losses.cl1_loss(fusion(lrs, alphas), hrs, maps).mean()
        loss.backward()
        optimizer.step()
        seen.append(float(loss.detach()))
    assert np.isfinite(seen).all() and not built
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, fusion.parameters()))
