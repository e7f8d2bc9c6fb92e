"""CPU: the fp64 references of tests/test_gpu_kernels_bwd.py against torch autograd (float64) of the forward operation each is the gradient
of, and the claims that file makes about its own inputs (the decoder's `up` exact in fp32 with zeros present; ties at most pixels of the
routing inputs; exact zeros of both signs in the PReLU's stored tensor; the bf16 ties in the split inputs)."""
import pytest
import torch
import torch.nn.functional as F

import kernel_refs as K

D = torch.float64


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=D)


def _close(got, want, tol=1e-12):
    assert got.shape == want.shape, (got.shape, want.shape)
    assert float((got - want).abs().max()) <= tol * (1.0 + float(want.abs().max())), float((got - want).abs().max())


@pytest.mark.parametrize("a", K.PRELU_SLOPES)
def test_prelu_bwd_reference(a):
    """F.prelu after a conv bias: g = d (x + b), db, dslope; from the stored y when a > 0, from the pre-activation otherwise"""
    rows, Cc = 37, 64
    x0 = _rand((rows, Cc), 1)
    x0.view(-1)[::5] = 0.0
    b = torch.zeros(Cc, dtype=D, requires_grad=True)
    sl = torch.tensor([a], dtype=D, requires_grad=True)
    xin = x0.clone().requires_grad_(True)
    pre = xin + b
    y = F.prelu(pre, sl)
    dy = _rand((rows, Cc), 2)
    (y * dy).sum().backward()
    src = y.detach() if a > 0 else pre.detach()
    g, dslope, Ts, db, Tb = K.ref_prelu_bwd(dy, src, a)
    _close(g, xin.grad)
    _close(db, b.grad)
    _close(dslope.reshape(1), sl.grad, 1e-9)        # (y / a with a = 2^-20 is exact; 1.5 is not)
    assert float(Ts) >= abs(float(dslope)) and bool((Tb >= db.abs()).all())


@pytest.mark.parametrize("n", K.LEVELS + [3])
@pytest.mark.parametrize("ar", [0, 1])
def test_fusion_level_references(n, ar):
    """the fusion-level formula of oracle/torch_port.py (alice + alpha_bob f, flipped partners, odd level) with f an elementwise function of
    the pair gather z: ref_fuse_update is its forward, ref_fuse_df / ref_fuse_scatter / ref_alpha_grad its gradients"""
    B, hw = 3, 5
    half, parity, pair_last, V = n // 2, n % 2, n - (n & 1) - 1, n + 2
    x = _rand((B, n, hw, 64), 3).requires_grad_(True)
    alphas = K._alphas(B, V).double().requires_grad_(True)
    p, q = _rand((hw, 64), 4), _rand((hw, 64), 5)
    alice = x[:, :half]
    bob = x[:, half:n - parity].flip(1)
    z = torch.cat([alice, bob], -1)
    f = z[..., :64] * p + z[..., 64:] * q
    f.retain_grad()
    if ar:
        a_bob = alphas[:, half:n - parity].flip(1).reshape(B, half, 1, 1)
        out = alice + a_bob * f
    else:
        out = f
    dsn = _rand((B, half, hw, 64), 6)
    (out * dsn).sum().backward()
    up, T = K.ref_fuse_update(x.detach(), f.detach(), alphas.detach(), pair_last, ar)
    _close(up, out.detach())
    df, _ = K.ref_fuse_df(dsn, alphas.detach(), pair_last, ar)
    _close(df, f.grad)
    dz = torch.cat([df * p, df * q], -1)
    ds, T = K.ref_fuse_scatter(dsn, dz, n, pair_last, ar)
    _close(ds, x.grad)
    if parity:
        assert bool((ds[:, n - 1] == 0).all())
    if ar:
        da, _ = K.ref_alpha_grad(dsn, f.detach())
        want = torch.zeros((B, V), dtype=D)
        want[:, pair_last - torch.arange(half)] = da
        _close(want, alphas.grad)
        wrong, _ = K.ref_fuse_df(dsn, alphas.detach(), pair_last, ar, own_alpha=True)
        assert float((wrong - f.grad).abs().max()) > 1e-3
    wrong, _ = K.ref_fuse_scatter(dsn, dz, n, pair_last, ar, swap_halves=True)
    assert float((wrong - x.grad).abs().max()) > 1e-3


@pytest.mark.parametrize("S", [2, 3, 4])
@pytest.mark.parametrize("a", K.DEC_SLOPES)
def test_decoder_bwd_reference(S, a):
    """conv_transpose2d -> prelu -> 1 x 1 conv, on the GPU test's own inputs (so `up == 0` occurs: the slope's branch there)"""
    N, H, W = 2, 3, 5
    fused, d_sr, wd, bd, wf = [t.double() for t in K.decoder_inputs(N, H, W, S, 7 + S)]
    leaves = [t.clone().requires_grad_(True) for t in (fused, wd, bd, wf)]
    sl = torch.tensor([a], dtype=D, requires_grad=True)
    bf = torch.zeros(1, dtype=D, requires_grad=True)
    up = F.conv_transpose2d(K._nchw(leaves[0]), leaves[1], leaves[2], stride=S)
    assert bool((up == 0).any())
    sr = F.conv2d(F.prelu(up, sl), leaves[3].view(1, 64, 1, 1), bf)[:, 0]
    (sr * d_sr).sum().backward()
    ref = K.ref_decoder_bwd(fused, d_sr, wd, bd, a, wf, S)
    for name, want in (("d_fused", leaves[0].grad), ("dwd", leaves[1].grad), ("dbd", leaves[2].grad), ("dad", sl.grad.reshape(())),
                       ("dwf", leaves[3].grad), ("dbf", bf.grad.reshape(()))):
        _close(ref[name][0], want)
        assert bool((ref[name][1] >= ref[name][0].abs() - 1e-12).all())
    if S == 3:
        assert float((K.ref_decoder_bwd(fused, d_sr, wd, bd, a, wf, S, transpose_taps=True)["d_fused"][0] - leaves[0].grad).abs().max()) > 1e-3


@pytest.mark.parametrize("S", [2, 3, 4])
def test_decoder_up_is_exact_in_fp32(S):
    """the decoder inputs' claim: `up` evaluated in fp32 in two different orders (torch's, and the kernel's four 16-channel partial sums
    with the bias last, channels reversed) equals the fp64 value bit for bit, and up == 0 occurs"""
    N, H, W = 3, 9, 27
    fused, _, wd, bd, _ = K.decoder_inputs(N, H, W, S, 900 + 10 * S + N)
    up64 = K.ref_decoder_up(fused.double(), wd.double(), bd.double(), S)
    up32 = F.conv_transpose2d(K._nchw(fused), wd, bd, stride=S)
    assert up32.dtype == torch.float32 and torch.equal(up32.double(), up64)
    parts = [F.conv_transpose2d(K._nchw(fused[..., 16 * q:16 * q + 16].flip(-1)), wd[16 * q:16 * q + 16].flip(0), None, stride=S) for q in range(4)]
    alt = bd.view(1, 64, 1, 1) + ((parts[0] + parts[1]) + (parts[2] + parts[3]))
    assert alt.dtype == torch.float32 and torch.equal(alt.double(), up64)
    assert int((up64 == 0).sum()) >= 32 and bool((up64 > 0).any()) and bool((up64 < 0).any())
    assert float(up64.abs().max()) < 64.0


def _stem_forward(lrs, w, b):
    B, V, H, W = lrs.shape
    ref = torch.median(lrs[:, :9], 1, keepdim=True).values
    x = torch.stack([lrs, ref.expand(-1, V, -1, -1)], 2).reshape(B * V, 2, H, W)
    return F.conv2d(x, w, b, padding=1), ref[:, 0]


@pytest.mark.parametrize("V", [1, 2, 3, 8, 9, 10, 12])
def test_stem_references(V):
    """conv2d(cat(lr, ref)): the weight gradient, the pre-activation and, with distinct values (one view equals the median: torch's
    routing is then the rule's), the input gradient"""
    B, H, W = 2, 5, 7
    lrs = _rand((B, V, H, W), 8 + V).requires_grad_(True)
    w = (_rand((64, 2, 3, 3), 9) * 0.3).requires_grad_(True)
    b = _rand((64,), 10)
    pre, ref = _stem_forward(lrs, w, b)
    dA = _rand((B * V, H, W, 64), 11)
    (pre * K._nchw(dA)).sum().backward()
    x0, x1 = lrs.detach().reshape(B * V, H, W), ref.detach()
    got_pre, T = K.ref_stem_pre(x0, x1, V, w.detach(), b)
    _close(got_pre, pre.detach())
    dw, T = K.ref_stem_wgrad(x0, x1, V, None, dA, step=3)
    _close(dw, w.grad)
    d_lrs, T = K.ref_stem_dgrad_route(dA, w.detach(), lrs.detach(), ref.detach())
    _close(d_lrs, lrs.grad)
    assert bool((T >= d_lrs.abs() - 1e-12).all())


@pytest.mark.parametrize("V", [1, 2, 3, 9, 10, 12])
def test_stem_dgrad_ref_reference(V):
    """conv2d(cat(lr, ref)) with `ref` a leaf of its own (the frame given from outside): d_lrs is channel 0 per view, d_ref channel 1 summed
    over ALL V views of the sample (no window of nine, unlike the median), at a ragged shape with two tile columns and three tile rows"""
    B, H, W = 2, 17, 50
    lrs = _rand((B, V, H, W), 20 + V).requires_grad_(True)
    ref = _rand((B, H, W), 21 + V).requires_grad_(True)
    w = _rand((64, 2, 3, 3), 22) * 0.3
    x = torch.stack([lrs, ref[:, None].expand(-1, V, -1, -1)], 2).reshape(B * V, 2, H, W)
    dA = _rand((B * V, H, W, 64), 23)
    (F.conv2d(x, w, None, padding=1) * K._nchw(dA)).sum().backward()
    d_lrs, T_lrs, d_ref, T_ref = K.ref_stem_dgrad_ref(dA, w, B, V)
    assert tuple(d_lrs.shape) == (B, V, H, W) and tuple(d_ref.shape) == (B, H, W)
    _close(d_lrs, lrs.grad)
    _close(d_ref, ref.grad)
    assert bool((T_lrs >= d_lrs.abs() - 1e-12).all()) and bool((T_ref >= d_ref.abs() - 1e-12).all())
    # the routed reference is this one with d_ref added at the routed view
    li, med = K.route_inputs(B, V, H, W, 71 + V)
    routed, Tr = K.ref_stem_dgrad_route(dA, w, li, med)
    sel = K.ref_route_index(li, med)[:, None]
    _close(routed, d_lrs.scatter_add(1, sel, d_ref[:, None]))
    _close(Tr, T_lrs.scatter_add(1, sel, T_ref[:, None]))
    # the wrong references of the GPU negative controls are wrong
    if V > 1:
        assert not torch.equal(K.ref_stem_dgrad_ref(dA, w, B, V, drop_last_view=True)[2], d_ref)
    sw = K.ref_stem_dgrad_ref(dA, w, B, V, swap_channels=True)
    assert not torch.equal(sw[0], d_lrs) and not torch.equal(sw[2], d_ref)


def test_stem_wgrad_reference_with_sub():
    """`sub` is subtracted inside the image only, before the zero padding (ShiftNet's mean-free input)"""
    M, H, W = 5, 4, 6
    x = _rand((M, 2, H, W), 12)
    sub = _rand((M, 2), 13)
    w = torch.zeros((64, 2, 3, 3), dtype=D, requires_grad=True)
    g = _rand((M, H, W, 64), 14)
    (F.conv2d(x - sub[:, :, None, None], w, None, padding=1) * K._nchw(g)).sum().backward()
    dw, _ = K.ref_stem_wgrad(x[:, 0], x[:, 1], 1, sub, g, step=2)
    _close(dw, w.grad)


@pytest.mark.parametrize("V", [2, 3, 8, 9, 10, 12])
def test_routing_rule_on_tied_inputs(V):
    """the GPU test's routing inputs: ties at more than half of the pixels (V = 2: about half); the routed view is the lowest-indexed of the first min(V, 9)
    equal to the median; whatever view autograd picks among the tied ones, the sum over each group of tied views is the same"""
    B, H, W = 2, 15, 33
    lrs, ref = K.route_inputs(B, V, H, W, 71 + V)
    n = min(V, 9)
    eq = lrs[:, :n] == ref[:, None]
    assert float((eq.sum(1) > 1).double().mean()) > (0.5 if V >= 3 else 0.4)       # (V = 2: two values tie at half of the pixels)
    sel = K.ref_route_index(lrs, ref)
    for bb, y, x in ((0, 0, 0), (1, 7, 20), (1, 14, 32), (0, 3, 3)):
        first = [i for i in range(n) if float(lrs[bb, i, y, x]) == float(ref[bb, y, x])][0]
        assert int(sel[bb, y, x]) == first
    assert bool((K.ref_route_index(lrs, ref, highest=True) != sel).any())
    l64 = lrs.double().requires_grad_(True)
    w = _rand((64, 2, 3, 3), 15) * 0.3
    pre, _ = _stem_forward(l64, w, None)
    dA = _rand((B * V, H, W, 64), 16)
    (pre * K._nchw(dA)).sum().backward()
    d_lrs, _ = K.ref_stem_dgrad_route(dA, w, lrs.double(), ref.double())
    # channel 0 alone where a view is not tied with the median; the tied views of a pixel share the reference frame's gradient
    tied = torch.zeros((B, V, H, W), dtype=torch.bool)
    tied[:, :n] = eq
    _close(torch.where(tied, torch.zeros_like(d_lrs), d_lrs), torch.where(tied, torch.zeros_like(d_lrs), l64.grad))
    _close((d_lrs * tied).sum(1), (l64.grad * tied).sum(1))


@pytest.mark.parametrize("V", list(range(1, 13)))
def test_median_reference(V):
    lrs = torch.randint(-3, 4, (2, V, 6, 7), generator=torch.Generator().manual_seed(V)).float()
    n = min(V, 9)
    want = lrs[:, :n].sort(1).values[:, (n - 1) // 2]
    assert torch.equal(K.ref_median(lrs), want)
    if n % 2 == 0:
        assert not torch.equal(K.ref_median(lrs, upper=True), want)


def test_input_construction():
    """exact zeros of both signs among values of both signs in the PReLU's stored tensor; the split inputs hold bf16 ties, denormal-range
    lo parts and both zeros, and truncating differs from rounding on them; 16-bit values split exactly"""
    for dt in (K.F32, K.BF16, K.BF16X3):
        dy, src = K.prelu_inputs(33, 64, dt, 1)
        z = src == 0
        assert bool((z & torch.signbit(src)).any()) and bool((z & ~torch.signbit(src)).any())
        assert bool((src > 0).any()) and bool((src < 0).any())
        t = K.rnd((100,), 2, dt)
        hi, lo = K.ref_split_planes(t)
        assert torch.equal(hi.double() + lo.double(), t.double())
        assert torch.equal(*[x.view(torch.int16) for x in (K.ref_split_planes((hi.float() + lo.float()))[1], lo)])
    v = K.split_inputs(8 * 257, 3)
    hi, lo = K.ref_split_planes(v)
    assert bool(((v.view(torch.int32) & 0xFFFF) == 0x8000).any())
    tiny = (lo.float().abs() < 2.0 ** -126) & (lo.float() != 0)
    assert bool(tiny.any()) and bool(((v == 0) & torch.signbit(v)).any())
    assert not torch.equal(K.ref_split_planes(v, truncate_hi=True)[0].view(torch.int16), hi.view(torch.int16))
    assert float((hi.double() + lo.double() - v.double()).abs().max()) <= float((2.0 ** -16 * v.double().abs()).max())
