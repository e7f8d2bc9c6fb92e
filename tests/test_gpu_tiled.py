"""GPU (-m gpu): tiled inference on the device.  hrn_tile_gather and hrn_tile_scatter are pure data movement, and the network's
per-pixel arithmetic does not depend on where a pixel sits in a frame, so everything that has a whole-frame HIP counterpart is
compared BIT FOR BIT (torch.equal): the two kernels with the rule in hrnet_hip/tiling.py on every path (16-byte rows, per-element
rows, clamped borders, window sub-ranges, an offset base pointer, every scale), HRNet.forward_tiled with the plain forward of the
whole square frame in every precision, the tiled self-ensemble with forward_ensemble, the `tile` attribute, and the tiled
evaluation.  Rectangular scenes have no whole-frame HIP forward: they are held to the CPU port with the bounds of
tests/test_gpu_parity.py."""
import copy

import numpy as np
import pytest
import torch

from hrnet_hip import augment, tiling
from oracle import synth, torch_port, weights
from util import _check                       # the parity bounds: FP32_GUARD, X3_REL, BF16_REL / BF16_PSNR
import util

pytestmark = pytest.mark.gpu


def _rand(shape, seed):
    return util.dev(np.random.Generator(np.random.PCG64(seed)).standard_normal(shape).astype(np.float32))


def _ranges(n):
    """The whole plan, and a first, a middle and a last sub-range."""
    return sorted({(0, n), (0, max(1, n // 3)), (n // 3, max(n // 3 + 1, 2 * n // 3)), (n - 1, n), (max(0, n - 3), n)})


def _core_mask(p, w0, w1, S):
    mask = torch.zeros((S * p.H, S * p.W), dtype=torch.bool)
    for w in p.windows[w0:w1]:
        mask[S * w.cy0:S * w.cy1, S * w.cx0:S * w.cx1] = True
    return mask.cuda()


# --------------------------------------------------------------------------- the two kernels
#   (2,3,40,56,32,12): W % 4 == 0, t % 4 == 0: aligned 16-byte rows, windows clamped at both far borders
#   (1,2,24,37,20,9):  W % 4 != 0: every row of a plane is aligned differently; 30 windows with 2-pixel cores
#   (2,9,48,33,33,15): one window along W, odd t: destination rows drift against their sources
GEOMETRIES = [(2, 3, 40, 56, 32, 12), (1, 2, 24, 37, 20, 9), (2, 9, 48, 33, 33, 15)]


@pytest.mark.parametrize("B,V,H,W,t,R", GEOMETRIES, ids=lambda v: str(v))
def test_gather_equals_the_rule(B, V, H, W, t, R):
    from hrnet_hip import binding
    p = tiling.plan(H, W, t, R)
    n = len(p.windows)
    assert binding.tile_count(H, W, t, R) == n
    x = _rand((B, V, H, W), 10 + H)
    for w0, w1 in _ranges(n):
        got = binding.tile_gather(x, t, R, w0, w1)
        assert tuple(got.shape) == (w1 - w0, B, V, t, t)
        assert torch.equal(got, tiling.gather(x, p.windows[w0:w1], t)), (w0, w1)
    assert torch.equal(torch.ops.hrnet_hip.tile_gather(x, t, R, 0, n), tiling.gather(x, p.windows, t))


@pytest.mark.parametrize("scale", [2, 3, 4])
@pytest.mark.parametrize("B,V,H,W,t,R", GEOMETRIES, ids=lambda v: str(v))
def test_scatter_equals_the_rule(B, V, H, W, t, R, scale):
    """Into a NaN-filled output: exactly the cores of the range become finite, with the rule's values; the whole plan fills it."""
    from hrnet_hip import binding
    S = scale
    p = tiling.plan(H, W, t, R)
    n = len(p.windows)
    srs = _rand((n, B, 1, S * t, S * t), 20 + H + S)
    for w0, w1 in _ranges(n):
        got = torch.full((B, 1, S * H, S * W), float("nan"), device="cuda")
        want = tiling.scatter(torch.full_like(got, float("nan")), srs[w0:w1], p.windows[w0:w1], t, S)
        assert binding.tile_scatter(got, srs[w0:w1].contiguous(), t, R, S, w0, w1) is got
        assert torch.equal(torch.isfinite(got), _core_mask(p, w0, w1, S).expand_as(got)), (w0, w1)
        assert torch.equal(got.nan_to_num(nan=-7.0), want.nan_to_num(nan=-7.0)), (w0, w1)
        if (w0, w1) == (0, n):
            assert torch.isfinite(got).all()
    out = torch.zeros((B, 1, S * H, S * W), device="cuda")
    assert torch.ops.hrnet_hip.tile_scatter(out, srs, t, R, S, 0, n) is None
    assert torch.equal(out, tiling.scatter(torch.zeros_like(out), srs, p.windows, t, S))


@pytest.mark.parametrize("B,V,H,W,t,R", GEOMETRIES[:2], ids=lambda v: str(v))
def test_base_pointers_offset_by_four_bytes(B, V, H, W, t, R):
    """Contiguous views that start 4 bytes into their allocations: sources and destinations that no longer share an alignment."""
    from hrnet_hip import binding
    p = tiling.plan(H, W, t, R)
    n, S = len(p.windows), 3
    x = _rand((B * V * H * W + 1,), 31)[1:].view(B, V, H, W)
    assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    assert torch.equal(binding.tile_gather(x, t, R, 0, n), tiling.gather(x, p.windows, t))
    srs = _rand((n * B * S * t * S * t + 1,), 32)[1:].view(n, B, 1, S * t, S * t)
    for off in (0, 1):                              # an offset source alone, then both offset
        got = torch.full((B * S * H * S * W + off,), float("nan"), device="cuda")[off:].view(B, 1, S * H, S * W)
        assert srs.data_ptr() % 16 == 4 and got.data_ptr() % 16 == 4 * off
        binding.tile_scatter(got, srs, t, R, S, 0, n)
        assert torch.equal(got, tiling.scatter(torch.empty_like(got), srs, p.windows, t, S))


def test_opcheck():
    ops = torch.ops.hrnet_hip
    x = _rand((2, 3, 40, 56), 1)
    for args in ((x, 32, 12, 0, 8), (x, 32, 12, 3, 5)):
        torch.library.opcheck(ops.tile_gather.default, args, test_utils=("test_schema", "test_faketensor"))
    out = torch.zeros((2, 1, 120, 168), device="cuda")
    for args in ((out, _rand((8, 2, 1, 96, 96), 2), 32, 12, 3, 0, 8), (out, _rand((2, 2, 1, 96, 96), 3), 32, 12, 3, 3, 5)):
        torch.library.opcheck(ops.tile_scatter.default, args, test_utils=("test_schema", "test_faketensor"))


# --------------------------------------------------------------------------- HRNet.forward_tiled
def _model(scale, precision, train=False, **extra):
    from DeepNetworks.HRNet import HRNet
    cfg = dict(copy.deepcopy(weights.HRNET_CONFIG), **extra)
    cfg["decoder"]["deconv"]["kernel_size"] = cfg["decoder"]["deconv"]["stride"] = scale
    st = weights.to_torch_state(weights.hrnet_state(1234))
    if scale != 3:
        rng = np.random.Generator(np.random.PCG64(1234 + 100 * scale))
        w = rng.standard_normal((64, 64, scale, scale)) * float(st["decode.deconv.0.weight"].std())
        st["decode.deconv.0.weight"] = torch.from_numpy(w.astype(np.float32))
    m = HRNet(cfg)
    m.load_state_dict(st)
    m.precision = precision
    m = m.cuda()
    return m.train() if train else m.eval()


_scenes = {}


def _scene(B, V, H, W):
    """Device (lrs, alphas) of a (B, V, H, W) scene, cut from a square synthetic one; made once, shared, never modified."""
    key = (B, V, H, W)
    if key not in _scenes:
        lrs, alphas, _ = synth.make_batch(300 + V + H, B, V, max(H, W), V)
        _scenes[key] = (util.dev(lrs[:, :, :H, :W]), util.dev(alphas))
    return _scenes[key]


def _plain(m, x, a):
    packed, dt = m.packed_parameters()
    return torch.ops.hrnet_hip.hrnet_forward(packed, dt, m._num_layers, bool(m.fuse.alpha_residual), x, a, m._scale)


SQUARE = [(2, 4, 56, 32), (1, 9, 48, 33), (1, 32, 80, 48)]          # (B, V, side, tile); the last: R = 21, five fusion levels, 49 windows of 6 x 6 cores
SQUARE_CASES = [(3, c) for c in SQUARE] + [(2, SQUARE[0]), (4, SQUARE[0])]


@pytest.mark.parametrize("prec", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("scale,case", SQUARE_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_forward_tiled_equals_the_whole_frame(scale, case, prec):
    """Square scenes: the tiled forward is the plain forward of the whole frame, bit for bit, however the windows are chunked."""
    B, V, side, tile = case
    x, a = _scene(B, V, side, side)
    m = _model(scale, prec)
    R = tiling.halo(m._num_layers, V)
    p = tiling.plan(side, side, tile, R)
    assert len(p.windows) == {56: 16, 48: 36, 80: 49}[side] and R == {4: 12, 9: 15, 32: 21}[V]      # ceil((side - 2R) / (tile - 2R)) ** 2
    with torch.no_grad():
        whole = _plain(m, x, a)
        for wpp in (1, 3, None):
            got = m.forward_tiled(x, a, tile, windows_per_pass=wpp)
            assert tuple(got.shape) == (B, 1, scale * side, scale * side) and not got.requires_grad
            print(f"x{scale} {prec} B={B} V={V} {side}x{side} tile {tile} windows_per_pass={wpp}: "
                  f"max |tiled - whole| {float((got - whole).abs().max()):.3e} (max |whole| {float(whole.abs().max()):.3e})")
            assert torch.equal(got, whole), (wpp, float((got - whole).abs().max()))


@pytest.mark.parametrize("prec", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("B,V,H,W,tile", [(2, 4, 40, 56, 32), (1, 2, 24, 37, 20)], ids=lambda v: str(v))
def test_forward_tiled_rectangular_against_the_cpu_port(B, V, H, W, tile, prec):
    """No whole-frame HIP forward exists for H != W: the reference is the CPU port on the whole rectangular frame, with the parity bounds."""
    x, a = _scene(B, V, H, W)
    key = ("port", B, V, H, W)
    if key not in _scenes:
        _scenes[key] = torch_port.hrnet_forward(x.cpu(), a.cpu(), weights.to_torch_state(weights.hrnet_state(1234))).numpy()
    m = _model(3, prec)
    with torch.no_grad():
        got = m.forward_tiled(x, a, tile)
        assert tuple(got.shape) == (B, 1, 3 * H, 3 * W)
        assert torch.equal(m.forward_tiled(x, a, tile, windows_per_pass=1), got)
    print(f"{prec} {H}x{W} tile {tile}: max-rel vs the CPU port {util.rel_err(got.cpu().numpy(), _scenes[key]):.3e}")
    _check(prec, got.cpu().numpy(), _scenes[key])


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_tiled_ensemble(prec):
    m = _model(3, prec)
    codes = augment.ensemble_codes("dihedral")
    with torch.no_grad():
        # square: forward_ensemble of the whole frame
        x, a = _scene(2, 4, 56, 56)
        want = m.forward_ensemble(x, a, "dihedral")
        for kw in ({}, {"windows_per_pass": 2, "members_per_pass": 3}):
            got = m.forward_tiled(x, a, 32, ensemble="dihedral", **kw)
            assert torch.equal(got, want), float((got - want).abs().max())
        assert torch.equal(m.forward_tiled(x, a, 32, ensemble="flip"), m.forward_ensemble(x, a, "flip"))
        # rectangular: the ensemble window by window, stated with tiling and augment in torch
        x, a = _scene(2, 4, 40, 56)
        p = tiling.plan(40, 56, 32, 12)
        n, t = len(p.windows), p.t
        wins = tiling.gather(x, p.windows, t).reshape(n * 2, 4, t, t)
        members = augment.expand(wins, codes).reshape(8 * n * 2, 4, t, t).contiguous()
        srs = _plain(m, members, a.repeat(8 * n, 1)).view(8, n, 2, 1, 3 * t, 3 * t)
        want = tiling.scatter(torch.empty((2, 1, 120, 168), device="cuda"), augment.mean_inverse(srs, codes), p.windows, t, 3)
        got = m.forward_tiled(x, a, 32, ensemble="dihedral")
        assert torch.equal(got, want), float((got - want).abs().max())
        assert not torch.equal(got, m.forward_tiled(x, a, 32)) and torch.isfinite(got).all()


def test_one_window_goes_straight_to_the_plain_op():
    m = _model(3, "fp32")
    x, a = _scene(2, 4, 56, 56)
    with torch.no_grad():
        assert torch.equal(m.forward_tiled(x, a, 56), _plain(m, x, a)) and torch.equal(m.forward_tiled(x, a), _plain(m, x, a))
        assert torch.equal(m.forward_tiled(x, a, 64, ensemble="flip"), m.forward_ensemble(x, a, "flip"))


def test_tile_attribute_and_config_key():
    m = _model(3, "fp32", tile=32)
    assert m.tile == 32
    sq, a = _scene(2, 4, 56, 56)
    rect, _ = _scene(2, 4, 40, 56)
    small = sq[:, :, :32, :32].contiguous()
    with torch.no_grad():
        assert torch.equal(m(sq, a), m.forward_tiled(sq, a, 32)) and torch.equal(m(sq, a), _plain(m, sq, a))
        assert torch.equal(m(rect, a), m.forward_tiled(rect, a, 32))
        assert torch.equal(m(small, a), _plain(m, small, a))                    # within the tile: the plain path
        m.ensemble = "flip"                                                     # the routed call honours the ensemble
        assert torch.equal(m(rect, a), m.forward_tiled(rect, a, 32, ensemble="flip"))
        assert torch.equal(m(sq, a), m.forward_ensemble(sq, a, "flip"))
        assert torch.equal(m(small, a), m.forward_ensemble(small, a, "flip"))
        m.ensemble = None
        m.tile = None                                                           # unset: the plain op, and the old refusal
        assert torch.equal(m(sq, a), _plain(m, sq, a))
        with pytest.raises(ValueError, match="square"):
            m(torch.zeros(1, 2, 8, 16, device="cuda"), torch.ones(1, 2, device="cuda"))


@pytest.mark.parametrize("prec", ["fp32", "bf16", "bf16x3"])
def test_training_branch_is_never_tiled(prec):
    """.train() with grad enabled: `tile` changes neither the output nor the gradients, bit for bit; graph-free, the same module tiles."""
    x, a = _scene(2, 4, 56, 56)
    m = _model(3, prec, train=True)
    base = m(x, a)
    assert base.requires_grad
    (base ** 2).sum().backward()
    want = [p.grad.clone() for p in m.parameters()]
    m.zero_grad(set_to_none=True)
    m.tile = 32
    out = m(x, a)
    assert out.requires_grad and torch.equal(out, base)
    (out ** 2).sum().backward()
    assert all(p.grad is not None and torch.equal(p.grad, g) for p, g in zip(m.parameters(), want))
    with pytest.raises(ValueError, match="square"):                             # a non-square input is still refused when training
        m(torch.zeros(1, 2, 8, 16, device="cuda"), torch.ones(1, 2, device="cuda"))
    with torch.no_grad():
        assert torch.equal(m(x, a), m.forward_tiled(x, a, 32))


def test_evaluate_tiled_equals_untiled():
    from hrnet_hip import validate
    m = _model(3, "fp32", train=True)
    sets = []
    for i in range(2):
        lrs, alphas, hrs = synth.make_batch(70 + i, 2, 4, 64, 4)
        maps = (np.random.Generator(np.random.PCG64(i)).random((2, 192, 192)) > 0.1).astype(np.float32)
        sets.append((util.dev(lrs), util.dev(alphas), util.dev(hrs), util.dev(maps), [f"imgset{2 * i + j:04d}" for j in range(2)]))
    table = {f"imgset{i:04d}": 45.0 + i for i in range(4)}
    for ensemble in (None, "flip"):
        want = validate.evaluate(m, sets, baseline_cpsnrs=table, ensemble=ensemble)
        got = validate.evaluate(m, sets, baseline_cpsnrs=table, ensemble=ensemble, tile=32)
        assert got.names == want.names and np.array_equal(got.cpsnr, want.cpsnr) and got.score == want.score
        assert validate.sharded_val_score(m, sets, baseline_cpsnrs=table, ensemble=ensemble, tile=32) == want.score
    assert m.training
