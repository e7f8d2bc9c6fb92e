"""GPU (-m gpu): hrn_upsample and hrn_upsample_backward (csrc/upsample.hip) against the fp64 restatement (tests/upsample_ref.py) under the
project's bound |got - want| <= C T, C = 1e-5 (tests/kernel_bounds.py), T the restatement's sum of absolute terms: every scale, both
cubics, planes on which every tap clamps and folds, scalar rows, one tile more and less than the kernels' tile; the three forms of
`base`; sentinels behind every output; reproducibility; independence of the batch; the adjoint identity; the dispatcher ops and their
autograd formula; and one case whose output passes 2^31 elements."""
import numpy as np
import pytest
import torch

import kernel_bounds as KB
import kt
import upsample_ref as R
import util
from hrnet_hip import binding

pytestmark = pytest.mark.gpu

TH, TW = binding.UPSAMPLE_TILE
# (planes, H, W).  The first four: every tap clamped, several virtual rows / columns folding onto one in the adjoint.  (2, 5, 7): S W is
# no multiple of 4 at S = 2, 3, so rows that start off a 16-byte boundary take the single stores.  The last three: one below, exactly at
# and one above two tiles per axis.
SHAPES = [(3, 1, 1), (2, 1, 6), (2, 2, 5), (2, 3, 3), (2, 5, 7), (2, 2 * TH - 1, 2 * TW - 1), (2, 2 * TH, 2 * TW), (2, 2 * TH + 1, 2 * TW + 1)]
SCALES = [2, 3, 4]
CUBICS = [-0.75, -0.5]
_ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)
_cases = {}


def _case(shape, scale):
    """(frames, base, g) numpy f32 of a shape: values in [-1, 1); the last plane of `frames` and of `g` is constant (even H + W) or holds
    a single 1 (odd), and with three planes the middle one is the other kind - a tap's weight can be read off the result.  Made once."""
    if (shape, scale) not in _cases:
        n, H, W = shape
        rng = np.random.Generator(np.random.PCG64(1000 * scale + 31 * H + W))
        f = rng.uniform(-1, 1, shape).astype(np.float32)
        g = rng.uniform(-1, 1, (n, scale * H, scale * W)).astype(np.float32)
        base = rng.uniform(-1, 1, g.shape).astype(np.float32)
        kinds = ["const", "one"] if (H + W) % 2 == 0 else ["one", "const"]
        for k, kind in zip(range(n - 1, 0, -1), kinds):
            for t, (h, w) in ((f, (H, W)), (g, (scale * H, scale * W))):
                t[k] = 0.625 if kind == "const" else 0.0
                if kind == "one":
                    t[k, h // 2, w - 1 if k % 2 else w // 2] = 1.0
        _cases[(shape, scale)] = (f, base, g)
    return _cases[(shape, scale)]


def _forward(f, scale, a, base=None, inplace=False):
    """hrn_upsample into a sentinel-guarded output; inplace: the output starts as `base` and is handed over as base too"""
    n, H, W = f.shape
    x = util.dev(f)
    out = KB.Guarded((n, scale * H, scale * W), v=torch.from_numpy(base) if inplace else None)
    b = None if base is None or inplace else util.dev(base)
    rc = kt.lib().hrn_upsample(kt._p(x), out.ptr if inplace else kt._p(b), out.ptr, n, H, W, scale, a, kt._stream())
    torch.cuda.synchronize()
    assert rc == 0, binding.load_library().hrn_last_error()
    assert out.guard_ok(), "a write outside the output"
    return out


def _backward(g, scale, a):
    n, SH, SW = g.shape
    x = util.dev(g)
    out = KB.Guarded((n, SH // scale, SW // scale))
    rc = kt.lib().hrn_upsample_backward(kt._p(x), out.ptr, n, SH // scale, SW // scale, scale, a, kt._stream())
    torch.cuda.synchronize()
    assert rc == 0, binding.load_library().hrn_last_error()
    assert out.guard_ok(), "a write outside the gradient"
    return out


def _close(tag, got, want, T):
    return KB._assert_close(tag, "f32", got.double(), torch.from_numpy(want), torch.from_numpy(T), layout="n y x")


@pytest.mark.parametrize("a", CUBICS)
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_forward_against_the_restatement(shape, scale, a):
    f, base, _ = _case(shape, scale)
    plain = _forward(f, scale, a)
    _close(f"forward {shape} x{scale} a={a}", plain.get(), R.forward(f, scale, a), R.t_forward(f, scale, a))
    want, T = R.forward(f, scale, a, base), R.t_forward(f, scale, a, base)
    apart, inplace = _forward(f, scale, a, base), _forward(f, scale, a, base, inplace=True)
    _close(f"forward + base {shape} x{scale} a={a}", apart.get(), want, T)
    _close(f"forward in place {shape} x{scale} a={a}", inplace.get(), want, T)
    # the three forms agree: the fused ones bit for bit, and with the add done by torch within one rounding of the sum
    assert torch.equal(apart.bits(), inplace.bits())
    added = plain.get() + torch.from_numpy(base)
    assert bool(((apart.get().double() - added.double()).abs() <= 2.0 ** -23 * added.double().abs()).all())
    for k in range(1, shape[0]):                                 # a constant plane stays constant: every phase's weights sum to 1
        if (f[k] == 0.625).all():
            assert np.abs(plain.get().numpy()[k] - 0.625).max() <= KB.C * R.t_forward(f[k], scale, a).max()


@pytest.mark.parametrize("a", CUBICS)
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_backward_against_the_restatement(shape, scale, a):
    _, _, g = _case(shape, scale)
    got = _backward(g, scale, a)
    _close(f"backward {shape} x{scale} a={a}", got.get(), R.adjoint(g, scale, a), R.t_adjoint(g, scale, a))


@pytest.mark.parametrize("scale", SCALES)
def test_two_runs_are_bit_equal_and_a_plane_does_not_depend_on_its_batch(scale):
    for shape in (SHAPES[2], SHAPES[4], SHAPES[7]):
        f, base, g = _case(shape, scale)
        fw, bw = _forward(f, scale, -0.75, base), _backward(g, scale, -0.75)
        assert torch.equal(fw.bits(), _forward(f, scale, -0.75, base).bits()) and torch.equal(bw.bits(), _backward(g, scale, -0.75).bits())
        for k in range(shape[0]):
            assert torch.equal(_forward(f[k:k + 1], scale, -0.75, base[k:k + 1]).get()[0], fw.get()[k]), (shape, k)
            assert torch.equal(_backward(g[k:k + 1], scale, -0.75).get()[0], bw.get()[k]), (shape, k)


@pytest.mark.parametrize("a", CUBICS)
@pytest.mark.parametrize("scale", SCALES)
def test_adjoint_identity_of_the_device_results(scale, a):
    for shape in SHAPES:
        f, _, g = _case(shape, scale)
        up, ad = _forward(f, scale, a).get().double().numpy(), _backward(g, scale, a).get().double().numpy()
        lhs, rhs = float((up * g).sum()), float((f * ad).sum())
        bound = KB.C * (float((R.t_forward(f, scale, a) * np.abs(g)).sum()) + float((np.abs(f) * R.t_adjoint(g, scale, a)).sum()))
        print(f"{shape} x{scale} a={a}: <up f, g> - <f, up^T g> = {lhs - rhs:.3e}, bound {bound:.3e}")
        assert abs(lhs - rhs) <= bound


def test_ops_pass_opcheck_and_their_gradients_are_the_restatements():
    ops = torch.ops.hrnet_hip
    checks = ("test_schema", "test_faketensor", "test_autograd_registration")
    shape, scale, a = SHAPES[5], 3, -0.5
    f, base, g = _case(shape, scale)
    x, b, d = util.dev(f), util.dev(base), util.dev(g)
    torch.library.opcheck(ops.upsample.default, (x, b, scale, a), test_utils=checks)
    torch.library.opcheck(ops.upsample.default, (x.clone().requires_grad_(True), None, 2, -0.75), test_utils=checks)
    torch.library.opcheck(ops.upsample.default, (x.clone().requires_grad_(True), b.clone().requires_grad_(True), scale, a), test_utils=checks)
    torch.library.opcheck(ops.upsample_backward.default, (d, shape[1], shape[2], scale, a), test_utils=checks)
    # the ops are the C entry points
    assert torch.equal(ops.upsample(x, b, scale, a).cpu(), _forward(f, scale, a, base).get())
    assert torch.equal(ops.upsample_backward(d, shape[1], shape[2], scale, a).cpu(), _backward(g, scale, a).get())
    # autograd: d_frames is the adjoint of the upstream gradient, d_base the upstream gradient itself; each only when asked for
    from hrnet_hip import upsample
    xr, br = x.clone().requires_grad_(True), b.clone().requires_grad_(True)
    out = upsample.upsample(xr.view(1, *shape), scale, a, base=br.view(1, *g.shape))
    assert tuple(out.shape) == (1,) + g.shape
    out.backward(d.view(1, *g.shape))
    _close("op d_frames", xr.grad.cpu(), R.adjoint(g, scale, a), R.t_adjoint(g, scale, a))
    assert torch.equal(br.grad, d)
    xr2 = x.clone().requires_grad_(True)
    upsample.upsample(xr2, scale, a, base=b).backward(d)
    assert torch.equal(xr2.grad, xr.grad) and b.grad is None
    br2 = b.clone().requires_grad_(True)
    upsample.upsample(x, scale, a, base=br2).backward(d)
    assert torch.equal(br2.grad, d) and x.grad is None


def test_baseline_is_the_upsampled_composite():
    from hrnet_hip import composite, upsample
    rng = np.random.Generator(np.random.PCG64(5))
    lrs = util.dev(rng.uniform(0, 1, (2, 11, 9, 12)).astype(np.float32))
    masks = util.dev((rng.uniform(0, 1, (2, 11, 9, 12)) < 0.7).astype(np.float32))
    alphas = util.dev(np.concatenate([np.ones((2, 8), np.float32), np.zeros((2, 3), np.float32)], 1))
    for scale in SCALES:
        got = upsample.baseline(lrs, alphas, masks, scale=scale, a=-0.5, n_ref=7)
        ref = composite.masked_composite(lrs, masks, alphas, n_ref=7, fill=False)[0]
        assert tuple(got.shape) == (2, 1, scale * 9, scale * 12) and torch.equal(got[:, 0], upsample.upsample(ref, scale, -0.5))
    med = torch.median(lrs[:, :9], 1).values
    assert torch.equal(upsample.baseline(lrs)[:, 0], upsample.upsample(med, 3))


def test_output_beyond_2_31_elements():
    """57 planes of 2048 x 2048 at x3: 57 x 6144^2 = 2.15e9 output elements (past 2^31) in 8.6e9 bytes (past 2^32), 467k tiles walked by a
    grid of 2^16 workgroups.  Checked: plane 0, the last plane and the plane every boundary falls into, against the restatement formed in
    fp64 on the device (its matrices are tests/upsample_ref.py's)."""
    n, side, scale, a = 57, 2048, 3, -0.75
    KB._need(12)
    pool = KB._Pool()
    try:
        per = (scale * side) ** 2
        assert n * per > 1 << 31 and 4 * n * per > 1 << 32
        frames = pool.big(n, (side, side), KB.F32, fill="rand", seed=11, scale=0.5)
        out = pool.big(n, (scale * side, scale * side), KB.F32, fill="sent")
        before = frames.checksum()
        rc = kt.lib().hrn_upsample(frames.ptr, None, out.ptr, n, side, side, scale, a, kt._stream())
        torch.cuda.synchronize()
        assert rc == 0, binding.load_library().hrn_last_error()
        assert out.guards_intact() and frames.guards_intact() and frames.checksum() == before
        M = pool.keep(torch.from_numpy(R.axis_matrix(side, scale, a)).cuda())
        planes = KB.boundary_images(n, per, 4)
        assert planes[0] == 0 and planes[-1] == n - 1 and len(planes) >= 4
        for k in planes:
            f = frames.raw[2 * k * side * side:2 * (k + 1) * side * side].view(torch.float32).view(side, side).double()
            want, T = M @ f @ M.T, M.abs() @ f.abs() @ M.abs().T
            got = out.raw[2 * k * per:2 * (k + 1) * per].view(torch.float32).view(scale * side, scale * side).double()
            ratio = float(((got - want).abs() / (KB.C * T + 1e-300)).max())
            print(f"plane {k}: max error / bound {ratio:.3e}; C needed {ratio * KB.C:.2e}")
            assert ratio <= 1.0, k
            del f, want, T, got
    finally:
        pool.free()
