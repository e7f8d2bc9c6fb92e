"""The fp64 references of the per-element kernel tests and the inputs they are evaluated at: each ref_* function restates in fp64, on the
exact values a kernel reads, what the kernel computes, and returns with it T = the same expression on absolute values.
tests/test_gpu_kernels_bwd.py and tests/test_gpu_kernels_shiftnet.py hold the kernels to them on the GPU; tests/test_kernels_bwd_host.py
and tests/test_kernels_shiftnet_host.py check the references themselves against torch autograd / torch.optim.Adam on the CPU, on the same
inputs and constants, which is why those live here too.  The fp32 forward kernels' section serves tests/test_gpu_kernels_fwd.py (GPU)
and tests/test_kernels_fwd_f32_host.py (CPU) in the same way: the instances, the two operand sets, the references and the negative
controls of conv3x3_kernel<F32>, stem_kernel<F32> and decoder_kernel<F32, false, S>."""
import numpy as np
import torch
import torch.nn.functional as F

from kt import BF16, BF16X3, F32                        # noqa: F401
from kernel_bounds import BF, C, C_F32, SHAPES, _full32, _grid, _nchw, _pair_gather, _tiles, rnd, round_sig, sig_bits    # noqa: F401
# (the host tests reach the conventions through this module)

# ----------------------------------------------------------------------------------------------------------- HRNet's backward
def ref_prelu_bwd(dy, src, a, zero_is_positive=False, no_inv=False):
    """PReLU backward + bias gradient.  dy, src (rows, C) fp64; src = the stored post-activation y when a > 0, else the pre-activation.
    -> g, dslope, sum |dslope terms|, db, sum |db terms|.  At zero the derivative is the slope's branch (x > 0 ? dy : a dy)."""
    pos = src >= 0 if zero_is_positive else src > 0
    g = torch.where(pos, dy, a * dy)
    x = src / a if (a > 0 and not no_inv) else src
    t = torch.where(pos, torch.zeros_like(dy), dy * x)
    return g, t.sum(), t.abs().sum(), g.sum(0), g.abs().sum(0)


def _partner_alpha(alphas, half, pair_last, own=False):
    i = torch.arange(half)
    return (alphas[:, i] if own else alphas[:, pair_last - i]).double()[:, :, None, None]


def ref_fuse_update(stack, f, alphas, pair_last, alpha_residual):
    """stack (B, n, hw, 64), f (B, half, hw, 64), alphas (B, V) -> the kept views s_i + alpha[partner(i)] f_i (or f), and T"""
    half = f.shape[1]
    if not alpha_residual:
        return f.clone(), f.abs()
    al = _partner_alpha(alphas, half, pair_last)
    return stack[:, :half] + al * f, stack[:, :half].abs() + al.abs() * f.abs()


def ref_fuse_df(dsn, alphas, pair_last, alpha_residual, own_alpha=False):
    """dsn (B, half, hw, 64) -> d f = alpha[partner] dsn (or dsn), and T"""
    if not alpha_residual:
        return dsn.clone(), dsn.abs()
    al = _partner_alpha(alphas, dsn.shape[1], pair_last, own_alpha)
    return al * dsn, al.abs() * dsn.abs()


def ref_fuse_scatter(dsn, dz, n, pair_last, alpha_residual, swap_halves=False):
    """dsn (B, half, hw, 64), dz (B, half, hw, 128) -> d views (B, n, hw, 64): view i < half gets dz[..., :64] (+ dsn with the alpha
    residual), view pair_last - i gets dz[..., 64:] of image i, the unpaired view of an odd level exact zeros; and T"""
    B, half, hw, _ = dsn.shape
    lo, hi = (dz[..., 64:], dz[..., :64]) if swap_halves else (dz[..., :64], dz[..., 64:])
    ds = torch.zeros((B, n, hw, 64), dtype=torch.float64)
    T = torch.zeros_like(ds)
    ds[:, :half], T[:, :half] = lo, lo.abs()
    if alpha_residual:
        ds[:, :half] += dsn
        T[:, :half] += dsn.abs()
    i = torch.arange(half)
    ds[:, pair_last - i], T[:, pair_last - i] = hi, hi.abs()
    return ds, T


def ref_pair_add(stack, u, pair_last):
    """stack (B, n, hw, 64), u (B, half, hw, 128) -> t2 = cat(view v, view pair_last - v) + u, and T"""
    half = u.shape[1]
    v = torch.arange(half)
    z = torch.cat([stack[:, v], stack[:, pair_last - v]], -1)
    return z + u, z.abs() + u.abs()


def ref_alpha_grad(dsn, f):
    """dsn, f (B, half, hw, 64) -> sum over pixels and channels of dsn f per (b, v) (it belongs to d_alphas[b][pair_last - v]), and T"""
    p = dsn * f
    return p.sum((2, 3)), p.abs().sum((2, 3))


def _stem_input(x0, x1, rep1, sub, m0, m1):
    """images m0..m1 of the stem's two-channel input: (view m, frame m // rep1), `sub` [M][2] subtracted inside the image"""
    a, b = x0[m0:m1], x1[torch.arange(m0, m1) // rep1]
    if sub is not None:
        a, b = a - sub[m0:m1, 0, None, None], b - sub[m0:m1, 1, None, None]
    return torch.stack([a, b], 1)


def ref_stem_wgrad(x0, x1, rep1, sub, g, step=256):
    """x0 (M, H, W), x1 (ceil(M / rep1), H, W), g (M, H, W, 64) fp64 -> dw (64, 2, 3, 3) of conv2d(cat(x0, x1), pad 1), and T; in chunks of images"""
    M = x0.shape[0]
    dw = torch.zeros((64, 2, 3, 3), dtype=torch.float64)
    T = torch.zeros_like(dw)
    for m0 in range(0, M, step):
        m1 = min(M, m0 + step)
        z, gg = _stem_input(x0, x1, rep1, sub, m0, m1), _nchw(g[m0:m1])
        dw += torch.nn.grad.conv2d_weight(z, (64, 2, 3, 3), gg, padding=1)
        T += torch.nn.grad.conv2d_weight(z.abs(), (64, 2, 3, 3), gg.abs(), padding=1)
    return dw, T


def ref_stem_pre(x0, x1, rep1, w, b):
    """the stem's pre-activation (M, 64, H, W) and T"""
    z = _stem_input(x0, x1, rep1, None, 0, x0.shape[0])
    return F.conv2d(z, w, b, padding=1), F.conv2d(z.abs(), w.abs(), b.abs(), padding=1)


def ref_route_index(lrs, ref, highest=False):
    """lrs (B, V, H, W), ref (B, H, W) -> the view (B, H, W) that receives the reference frame's gradient: the lowest-indexed of the
    first min(V, 9) views equal to the median"""
    n = min(lrs.shape[1], 9)
    eq = lrs[:, :n] == ref[:, None]
    idx = torch.arange(n)[None, :, None, None].expand_as(eq)
    if highest:
        return torch.where(eq, idx, torch.full_like(idx, -1)).amax(1)
    return torch.where(eq, idx, torch.full_like(idx, n)).amin(1)


def ref_stem_dgrad_route(dA, w, lrs, ref, highest=False):
    """dA (B V, H, W, 64), w (64, 2, 3, 3) fp64 -> d_lrs (B, V, H, W) = channel 0 of conv_transpose(dA) per view plus, at the routed
    view, channel 1 summed over the sample's views; and T"""
    B, V, H, W = lrs.shape
    d, Ta = _stem_dgrad_both(dA, w, B, V)
    out, T = d[:, :, 0].clone(), Ta[:, :, 0].clone()
    sel = ref_route_index(lrs, ref, highest)[:, None]
    out.scatter_add_(1, sel, d[:, :, 1].sum(1, keepdim=True))
    T.scatter_add_(1, sel, Ta[:, :, 1].sum(1, keepdim=True))
    return out, T


def _stem_dgrad_both(dA, w, B, V):
    """dA (B V, H, W, 64), w (64, 2, 3, 3) fp64 -> the stem's input gradient (B, V, 2, H, W), both channels per view, and the same
    expression on absolute values"""
    H, W = dA.shape[1:3]
    d = torch.nn.grad.conv2d_input((B * V, 2, H, W), w, _nchw(dA), padding=1).reshape(B, V, 2, H, W)
    Ta = torch.nn.grad.conv2d_input((B * V, 2, H, W), w.abs(), _nchw(dA).abs(), padding=1).reshape(B, V, 2, H, W)
    return d, Ta


def ref_stem_dgrad_ref(dA, w, B, V, drop_last_view=False, swap_channels=False):
    """The stem's input gradient with the frame given from outside: dA (B V, H, W, 64), w (64, 2, 3, 3) fp64 ->
    (d_lrs (B, V, H, W), T_lrs, d_ref (B, H, W), T_ref): d_lrs channel 0 per view, d_ref channel 1 summed over the sample's V views, each T
    the same expression on absolute values.  drop_last_view / swap_channels: the wrong references of the negative controls"""
    d, Ta = _stem_dgrad_both(dA, w, B, V)
    c0, c1 = (1, 0) if swap_channels else (0, 1)
    n = V - 1 if drop_last_view else V
    return d[:, :, c0].clone(), Ta[:, :, c0].clone(), d[:, :n, c1].sum(1), Ta[:, :n, c1].sum(1)


def ref_decoder_up(fused, wd, bd, S):
    return F.conv_transpose2d(_nchw(fused), wd, bd, stride=S)


def ref_decoder_bwd(fused, d_sr, wd, bd, a, wf, S, transpose_taps=False):
    """fused (N, H, W, 64), d_sr (N, S H, S W), wd (64 ci, 64 co, S, S), bd (64), a, wf (64), all fp64 -> dict name -> (value, T) of
    d_fused (N, H, W, 64), dwd, dbd, dad, dwf, dbf of sr = conv1x1(PReLU(conv_transpose(fused)))"""
    if transpose_taps:
        wd = wd.transpose(2, 3).contiguous()
    z = _nchw(fused)
    up = ref_decoder_up(fused, wd, bd, S)
    ds = d_sr[:, None]
    dy = wf.view(1, 64, 1, 1) * ds
    pos = up > 0
    dup = torch.where(pos, dy, a * dy)
    y = torch.where(pos, up, a * up)
    neg = torch.where(pos, torch.zeros_like(up), dy * up)
    return {
        "d_fused": (F.conv2d(dup, wd, stride=S).permute(0, 2, 3, 1), F.conv2d(dup.abs(), wd.abs(), stride=S).permute(0, 2, 3, 1)),
        "dwd": (torch.nn.grad.conv2d_weight(dup, wd.shape, z, stride=S), torch.nn.grad.conv2d_weight(dup.abs(), wd.shape, z.abs(), stride=S)),
        "dbd": (dup.sum((0, 2, 3)), dup.abs().sum((0, 2, 3))),
        "dad": (neg.sum(), neg.abs().sum()),
        "dwf": ((y * ds).sum((0, 2, 3)), (y * ds).abs().sum((0, 2, 3))),
        "dbf": (ds.sum(), ds.abs().sum()),
    }


def ref_split_planes(v, truncate_hi=False):
    """f32 tensor -> (hi, lo) bf16: hi = bf16(v) round to nearest even, lo = bf16(v - hi)"""
    if truncate_hi:
        hi = (v.view(torch.int32) & ~0xFFFF).view(torch.float32).to(torch.bfloat16)
    else:
        hi = v.to(torch.bfloat16)
    return hi, (v - hi.float()).to(torch.bfloat16)


def ref_median(lrs, upper=False):
    """lrs (B, V, H, W) -> the lower median of the first min(V, 9) views"""
    x = lrs[:, :min(lrs.shape[1], 9)]
    if upper:
        return x.sort(1).values[:, x.shape[1] // 2]
    return torch.median(x, 1).values


def prelu_inputs(rows, Cc, dt, seed):
    """dy and the PReLU's stored tensor (y or the pre-activation): both signs, exact +0 and -0"""
    dy, src = rnd((rows, Cc), seed, dt), rnd((rows, Cc), seed + 1, dt)
    flat = src.view(-1)
    flat[::7] = 0.0
    flat[3::11] = -0.0
    return dy, src


def decoder_inputs(N, H, W, S, seed):
    """fused in k / 16 (|k| <= 32), wd in k / 64 (|k| <= 16), bd in k / 1024 (|k| <= 1024): every product is a multiple of 2^-10 of size <=
    1/2 and a sum of 64 plus the bias stays below 2^6, so `up` has 16 significant bits at most and is exact in fp32 in any order.
    Pixel 0 is the unit vector of channel 0 and bd[co] = -wd[0][co][0][0] at the even co: up == 0 exactly there.  d_sr, wf general."""
    g = torch.Generator().manual_seed(seed)
    fused = torch.randint(-32, 33, (N, H, W, 64), generator=g).float() / 16
    wd = torch.randint(-16, 17, (64, 64, S, S), generator=g).float() / 64
    bd = torch.randint(-1024, 1025, (64,), generator=g).float() / 1024
    fused[0, 0, 0] = 0
    fused[0, 0, 0, 0] = 1.0
    bd[::2] = -wd[0, ::2, 0, 0]
    d_sr = torch.randn((N, S * H, S * W), generator=g)
    wf = torch.randn(64, generator=g) * 0.2
    return fused, d_sr, wd, bd, wf


def route_inputs(B, V, H, W, seed):
    """lrs of small integers 0..3 (0..1 for V <= 3, where four values would rarely tie) and their median: the median is tied between
    views at more than half of the pixels for V >= 3, at about half of them for V = 2"""
    lrs = torch.randint(0, 2 if V <= 3 else 4, (B, V, H, W), generator=torch.Generator().manual_seed(seed)).float()
    return lrs, ref_median(lrs)


def split_inputs(n, seed):
    """fp32 values for f32_to_planes: random, ties of the bf16 rounding (low half 0x8000 under an even and an odd hi), their neighbours,
    values whose lo part lies in bf16's denormal range, +0 and -0"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(n, generator=g)
    bits = v.view(torch.int32)
    pat = torch.tensor([0x8000, 0x18000, 0x7FFF, 0x8001, 0x17FFF, 0x18001], dtype=torch.int32)
    k = torch.arange(0, n, 3)
    bits[k] = (bits[k] & ~0x1FFFF) | pat[(k // 3) % 6]
    v[1::16] = v[1::16] * 2.0 ** -118          # lo around 2^-127 and below: bf16 denormals
    v[5::64] = 0.0
    v[6::64] = -0.0
    return v


# the slopes, fusion levels and alphas both the GPU tests and the host checks of the references run
PRELU_SLOPES = [0.25, 1.0, 1.5, 2.0 ** -20, 0.0, BF(-0.3)]
DEC_SLOPES = [0.25, 0.0, BF(-0.3), 1.5, 1.0]
ALPHA_PATTERN = [0.0, 1.0, 0.75, 0.75, 1.0, 0.0, 0.75]
LEVELS = [2, 5, 6, 9]


def _alphas(B, V, zero_at=None):
    """alphas (B, V) mixed 0 / 1 / 0.75 per sample; zero_at: a slot of the last sample set to 0 (the partner of view 0: every case then has
    an alpha = 0 output)"""
    al = torch.tensor([[ALPHA_PATTERN[(b + j) % 7] for j in range(V)] for b in range(B)], dtype=torch.float32)
    if zero_at is not None:
        al[B - 1, zero_at] = 0.0
    return al


# ----------------------------------------------------------------------------------------------------------- the fp32 forward kernels
# tests/test_gpu_kernels_fwd.py holds conv3x3_kernel<F32>, stem_kernel<F32> and decoder_kernel<F32, false, S> to these on the GPU;
# tests/test_kernels_fwd_f32_host.py checks on the CPU, with the same seeds, that the `full` operands carry more than 16 significant
# bits, that a float32 evaluation stays inside the bound and that every asserted negative control is further from the right reference
# than the bound can hide.
# instance: (dt, route, cin, cout, res_mode, in_pair, slot output); F32 reaches conv3x3_kernel<F32, cin, cout> on route 0 and on route 1
F32_INSTANCES = {
    "f32enc": (F32, 0, 64, 64, 0, False, False),
    "f32encres": (F32, 0, 64, 64, 1, False, False),
    "f32pairin": (F32, 0, 128, 128, 0, True, False),
    "f32pairres": (F32, 0, 128, 128, 2, False, False),
    "f32alpha": (F32, 0, 128, 64, 3, False, "stack"),
    "f32alphalast": (F32, 0, 128, 64, 3, False, "fused"),
    "f32slot": (F32, 0, 128, 64, 0, False, "stack"),
    "f32slotlast": (F32, 0, 128, 64, 0, False, "fused"),
}
# slope classes: None (no PReLU), 0 <= a <= 1, 0, 1, a < 0, a > 1; the `full` set's are general fp32 values of the same classes
SLOPES = [None, 0.25, 0.0, 1.0, BF(-0.3), 1.5]
_F = lambda v: float(np.float32(v))
SLOPES_FULL = [None, _F(0.3), 0.0, 1.0, _F(-0.3), _F(1.7)]
ALPHA_FULL = _F(0.7)


def f32_slope(a, opset):
    """the slope an fp32 case runs with: the `full` set's value of the class of `a`"""
    return SLOPES_FULL[SLOPES.index(a)] if opset == "full" else a


def f32_opset(ii, si):
    """the operand set of fp32 instance number ii at shape number si: `full` at every odd shape (15x33 and multi among them) and where
    (ii + si) % 3 == 0, `exact` (bf16-representable values stored as f32: every product exact) at the other even shapes"""
    return "full" if si % 2 == 1 or (ii + si) % 3 == 0 else "exact"


def conv_geometry(inst, shape):
    """-> dict B, V, n, half, pair_last, per, M, uses_stack of instance tuple `inst` at `shape` (a key of SHAPES).  A level of n views
    (pair_last = n - 2 for odd n) inside a stack of V > n slots; "multi" (needs the GPU's CU count): a workgroup walks two tiles at least"""
    dt, route, cin, cout, res_mode, in_pair, slot = inst
    H, W = SHAPES[shape]
    uses_stack = bool(in_pair or res_mode in (2, 3) or slot)
    n = 3 if slot == "fused" else 5
    V = n + 2
    half, pair_last = n // 2, n - (n & 1) - 1
    per = half if uses_stack else 1
    tiles = _tiles(dt, route, cin, cout, H, W)
    if shape == "multi":
        B = 1
        while (B * per * tiles) < 2 * _grid(route, cout, B * per * tiles, dt):
            B += 1
        B += 1
    else:
        B = 2 if shape != "1x1" or uses_stack else 1
    M = B * per
    if shape == "multi":
        assert M * tiles >= 2 * _grid(route, cout, M * tiles, dt), (M * tiles, _grid(route, cout, M * tiles, dt))
    return dict(B=B, V=V, n=n, half=half, pair_last=pair_last, per=per, M=M, uses_stack=uses_stack, H=H, W=W)


def f32_values(shape, seed, scale, opset):
    """fp32 CPU values of operand set `exact` (bf16-representable) or `full` (general fp32)"""
    v = _full32(shape, seed, scale)
    return v.to(torch.bfloat16).float() if opset == "exact" else v


def f32_conv_operands(inst, geo, seed, opset):
    """the fp32 CPU operands of an F32 conv case: w (cout, cin, 3, 3), bias, and whichever of stack (B, V, H, W, 64), inp (M, H, W, cin),
    res (M, H, W, cout: res_mode 1, in place) the instance reads.  No operand holds a zero (an alpha = 0 slot is compared bit for bit with
    its residual, and -0.0 + 0 v is +0.0)."""
    _, _, cin, cout, res_mode, in_pair, slot = inst
    H, W = geo["H"], geo["W"]
    g = torch.Generator().manual_seed(seed)
    w = torch.randn((cout, cin, 3, 3), generator=g) * (0.05 if cin == 64 else 0.035)
    bias = torch.randn(cout, generator=g) * 0.1
    if opset == "exact":
        w, bias = w.to(torch.bfloat16).float(), bias.to(torch.bfloat16).float()
    ops = dict(w=w, bias=bias, stack=None, inp=None, res=None)
    if geo["uses_stack"]:
        ops["stack"] = f32_values((geo["B"], geo["V"], H, W, 64), seed + 1, 1.0, opset)
    if not in_pair:
        ops["inp"] = f32_values((geo["M"], H, W, cin), seed + 2, 1.0, opset)
    if res_mode == 1:
        ops["res"] = f32_values((geo["M"], H, W, cout), seed + 3, 1.0, opset)
    for t in ops.values():
        assert t is None or not bool((t == 0).any())
    return ops


def conv_alphas(B, V, opset="exact"):
    """alphas [B][V]: 0, 1, 0.75 (`full`: fp32(0.7)) mixed in the batch (the partner of slot i is pair_last - i)"""
    al = torch.tensor([[ALPHA_PATTERN[(b + j) % 7] for j in range(V)] for b in range(B)], dtype=torch.float32)
    return torch.where(al == 0.75, torch.full_like(al, ALPHA_FULL), al) if opset == "full" else al


def ref_prelu_fwd(x, T, a):
    if a is None:
        return x, T
    return torch.where(x >= 0, x, a * x), (None if T is None else T * max(1.0, abs(a)))


def ref_conv_epi(x, w, b, slope, res_mode, res=None, stack=None, geo=None, alph=None, own_alpha=False, swap_halves=False, with_T=True):
    """One conv3x3 layer with the epilogue of ConvParams, in the dtype of its arguments (fp64: the reference; fp32: a plain CPU evaluation):
    x (M, H, W, cin), w (cout, cin, 3, 3), b; PReLU `slope` (None: none); res_mode 1: + res (M, H, W, cout); 2: + the pair gather of
    stack[:, :n]; 3: stack slot i + alpha[partner(i)] conv (alph None: 1).  -> (M, cout, H, W) and T, the same on absolute values.
    The wrong references of the negative controls: own_alpha (the view's own alpha), swap_halves (res_mode 2's 64-channel halves exchanged)."""
    z = _nchw(x)
    y = F.conv2d(z, w, b, padding=1)
    T = F.conv2d(z.abs(), w.abs(), b.abs(), padding=1) if with_T else None
    y, T = ref_prelu_fwd(y, T, slope)
    add = lambda T, t: T + t if with_T else None
    if res_mode == 1:
        y, T = y + _nchw(res), add(T, _nchw(res).abs())
    elif res_mode == 2:
        st = stack[:, :geo["n"]]
        zz = _pair_gather(st, geo["half"], geo["pair_last"])
        if swap_halves:
            zz = torch.cat([zz[..., 64:], zz[..., :64]], -1)
        y, T = y + _nchw(zz), add(T, _nchw(zz).abs())
    elif res_mode == 3:
        half, M = geo["half"], x.shape[0]
        r = _nchw(stack[:, :half].reshape((M,) + tuple(stack.shape[2:])))
        if alph is None:
            al = torch.ones(M, dtype=y.dtype)
        else:
            i = torch.arange(half)
            al = (alph[:, i] if own_alpha else alph[:, geo["pair_last"] - i]).reshape(M).to(y.dtype)
        al = al[:, None, None, None]
        y, T = r + al * y, (r.abs() + al.abs() * T if with_T else None)
    return y, T


def ref_conv_rows(xpad, w, b, slope, res_mode=0, res=None, alpha=1.0):
    """Output rows y0..y1 of one image of a conv3x3 layer with the epilogue of ConvParams, from the rows the kernel reads for them:
    xpad (y1 - y0 + 2, W, cin) = input rows y0 - 1 .. y1, the REAL neighbour rows inside the image and zeros where they lie outside it (the
    convolution's padding); res (y1 - y0, W, cout): res_mode 1 the residual's rows, 2 the pair gather's, 3 the stack slot's (then
    res + alpha conv).  -> (cout, y1 - y0, W) and T.  With y0 = 0, y1 = H it is ref_conv_epi of the whole image."""
    z = xpad.permute(2, 0, 1)[None]
    y = F.conv2d(z, w, b, padding=(0, 1))
    T = F.conv2d(z.abs(), w.abs(), b.abs(), padding=(0, 1))
    y, T = ref_prelu_fwd(y, T, slope)
    if res_mode in (1, 2):
        r = res.permute(2, 0, 1)[None]
        y, T = y + r, T + r.abs()
    elif res_mode == 3:
        r = res.permute(2, 0, 1)[None]
        y, T = r + alpha * y, r.abs() + abs(alpha) * T
    return y[0], T[0]


def ref_conv_dgrad(g, w, res=None):
    """g (M, H, W, cout), raw weights w (cout, cin, 3, 3) fp64 -> dx (M, cin, H, W) = the input gradient of conv2d(x, w, padding=1)
    (+ res (M, H, W, cin)), and T"""
    z = _nchw(g)
    dx, T = F.conv_transpose2d(z, w, padding=1), F.conv_transpose2d(z.abs(), w.abs(), padding=1)
    if res is not None:
        dx, T = dx + _nchw(res), T + _nchw(res).abs()
    return dx, T


def ref_conv_wgrad(x, g):
    """x (M, H, W, cin), g (M, H, W, cout) fp64 -> dw (cout, cin, 3, 3) of conv2d(x, w, padding=1), and T"""
    shape = (g.shape[-1], x.shape[-1], 3, 3)
    return (torch.nn.grad.conv2d_weight(_nchw(x), shape, _nchw(g), padding=1),
            torch.nn.grad.conv2d_weight(_nchw(x).abs(), shape, _nchw(g).abs(), padding=1))


def f32_stem_operands(mode, M, H, W, seed):
    """general fp32 operands of the fp32 stem (unlike the bf16 modes' k / 2^16 they are no 16-bit values): mode `f32` as encoder_impl calls
    it - x0 (M, H, W), x1 (ceil(M / 3), H, W), rep1 = 3, no `sub`; `f32sub` as ShiftNet's eval pass - one tensor x (M, 2, H, W) whose
    plane 0 / 1 are in0 / in1 (image stride 2 H W, rep1 = 1) and sub (M, 2) = the plane means.  w (64, 2, 3, 3), bias (64) general fp32."""
    g = torch.Generator().manual_seed(seed)
    if mode == "f32sub":
        x = torch.rand((M, 2, H, W), generator=g) + 0.25 * torch.randn((M, 2, 1, 1), generator=g)
        x0, x1, rep1 = x[:, 0], x[:, 1], 1
        sub = x.double().mean((2, 3)).float()
    else:
        rep1 = 3
        x, sub = None, None
        x0, x1 = torch.rand((M, H, W), generator=g), torch.rand((-(-M // rep1), H, W), generator=g)
    w = torch.randn((64, 2, 3, 3), generator=g) * 0.3
    bias = torch.randn(64, generator=g) * 0.1
    return dict(x=x, x0=x0, x1=x1, rep1=rep1, sub=sub, w=w, bias=bias)


def ref_stem_fwd(x0, x1, rep1, sub, w, b, slope, m0, m1, with_T=True):
    """images m0..m1 of the stem: PReLU(conv2d(cat(x0[m] - sub[m, 0], x1[m // rep1] - sub[m, 1]), pad 1) + b) (M, 64, H, W), and T"""
    z = _stem_input(x0, x1, rep1, sub, m0, m1)
    y = F.conv2d(z, w, b, padding=1)
    T = F.conv2d(z.abs(), w.abs(), b.abs(), padding=1) if with_T else None
    return ref_prelu_fwd(y, T, slope)


def f32_decoder_operands(N, H, W, S, seed):
    """general fp32 operands of the fp32 decoder: fused (N, H, W, 64), wd (64, 64, S, S), bd (64), wf (64), bf (1)"""
    g = torch.Generator().manual_seed(seed)
    return dict(fused=torch.randn((N, H, W, 64), generator=g), wd=torch.randn((64, 64, S, S), generator=g) * 0.05,
                bd=torch.randn(64, generator=g) * 0.1, wf=torch.randn(64, generator=g) * 0.2, bf=torch.randn(1, generator=g) * 0.1)


def ref_decoder_fwd(fused, wd, bd, slope, wf, bf, S, with_T=True):
    """sr (N, S H, S W) = conv1x1(PReLU(conv_transpose(fused, wd, stride S) + bd), wf) + bf, and T"""
    z = _nchw(fused)
    y = F.conv_transpose2d(z, wd, bd, stride=S)
    T = F.conv_transpose2d(z.abs(), wd.abs(), bd.abs(), stride=S) if with_T else None
    y, T = ref_prelu_fwd(y, T, slope)
    want = F.conv2d(y, wf.view(1, 64, 1, 1), bf)[:, 0]
    T = F.conv2d(T, wf.abs().view(1, 64, 1, 1), bf.abs())[:, 0] if with_T else None
    return want, T


# the fp32 negative controls, at 15x33 on the `full` operand set (the decoder, whose shape table has no 15x33, at 17x50 and S = 3).
# (control, target): target an F32 conv instance, "stem" or "decoder".
# Structural: tap_swap (two taps of one (co, ci) pair exchanged), own_alpha, swap_halves (res_mode 2's halves), swap_in (the pair-gather
# INPUT's 64-channel halves exchanged: the chunk -> src0 / src1 selection).  Operand rounding, of the activations (x) or the weights (w),
# to 8 (bf16), 11 (10 mantissa bits) or 16 significant bits (the bf16x3 class).
F32_CONTROL_SHAPE, F32_CONTROL_SEED, F32_CONTROL_SLOPE = "15x33", 321, 0.25
F32_CONTROL_DECODER = ("17x50", 3)            # (shape, S)
_CONV_ROUND = ("f32enc", "f32pairin", "f32slot")
F32_CONTROLS = ([("tap_swap", "f32encres"), ("tap_swap", "f32pairres"), ("own_alpha", "f32alpha"), ("swap_halves", "f32pairres"),
                 ("swap_in", "f32pairin")] +
                [(f"round{b}_{o}", n) for b in (8, 11) for o in ("x", "w") for n in _CONV_ROUND] +
                [("round16_x", "stem"), ("round8_x", "decoder")])
# Controls whose wrong reference is closer than twice the bound to the right one under C_F32, asserted nowhere (the host test prints their
# separation and fails if one of them clears 2): one operand of a convolution rounded to 16 significant bits moves the worst element by
# 1.2 (f32enc x), 1.1 (f32enc w), 0.73 .. 0.76 (f32pairin, f32slot) times C_F32 T, and the kernels themselves need up to 0.2 C_F32 T.
F32_CONTROLS_UNASSERTED = [(f"round16_{o}", n) for o in ("x", "w") for n in _CONV_ROUND]


def f32_control_reference(control, case):
    """the wrong reference of `control` (None: the right one): case = dict(kind "conv" / "stem" / "decoder", args: the keyword arguments
    of its ref_* function in fp64) -> (value, T)"""
    a = dict(case["args"])
    fn = {"conv": ref_conv_epi, "stem": ref_stem_fwd, "decoder": ref_decoder_fwd}[case["kind"]]
    xkey = {"conv": "x", "stem": None, "decoder": "fused"}[case["kind"]]
    wkey = {"conv": "w", "stem": "w", "decoder": "wd"}[case["kind"]]
    if control is None:
        pass
    elif control == "tap_swap":
        w = a["w"].clone()
        w[5, 7, 0, 0], w[5, 7, 2, 2] = a["w"][5, 7, 2, 2], a["w"][5, 7, 0, 0]
        assert w[5, 7, 0, 0] != w[5, 7, 2, 2]
        a["w"] = w
    elif control == "own_alpha":
        a["own_alpha"] = True
    elif control == "swap_halves":
        a["swap_halves"] = True
    elif control == "swap_in":
        a["x"] = torch.cat([a["x"][..., 64:], a["x"][..., :64]], -1)
    else:
        bits, which = int(control[5:control.index("_")]), control[-1]
        if which == "w":
            a[wkey] = round_sig(a[wkey], bits)
        elif case["kind"] == "stem":
            a["x0"], a["x1"] = round_sig(a["x0"], bits), round_sig(a["x1"], bits)
        else:
            a[xkey] = round_sig(a[xkey], bits)
    return fn(**a)


# ----------------------------------------------------------------------------------------------------------- ShiftNet and Adam
FCK = 32768                                   # fc1's K
EPS = float(np.float32(1e-5))                 # BatchNorm's eps as the kernels receive it
MOM = float(np.float32(0.1))                  # and the momentum
D = torch.float64


def ref_bn_stats(x, gamma, beta, rm, rv, unbiased_scale=False, biased_running=False):
    """BatchNorm2d in train mode over x (npix, C) fp64 -> name -> (value, T): mean, invstd = 1 / sqrt(biased var + eps), scale = gamma
    invstd, shift = beta - mean scale, and (rm given) the running statistics after one step of momentum MOM (unbiased variance)"""
    n = x.shape[0]
    mean, var = x.mean(0), x.var(0, unbiased=False)
    varu = var * n / (n - 1) if n > 1 else var
    invstd = 1.0 / torch.sqrt((varu if unbiased_scale else var) + EPS)
    scale = gamma * invstd
    out = dict(mean=(mean, mean.abs()), invstd=(invstd, invstd.abs()), scale=(scale, scale.abs()),
               shift=(beta - mean * scale, beta.abs() + (mean * scale).abs()))
    if rm is not None:
        stat = var if biased_running else varu
        out["running_mean"] = ((1 - MOM) * rm + MOM * mean, ((1 - MOM) * rm).abs() + (MOM * mean).abs())
        out["running_var"] = ((1 - MOM) * rv + MOM * stat, ((1 - MOM) * rv).abs() + (MOM * stat).abs())
    return out


def ref_bn_fold(gamma, beta, rm, rv, conv_bias):
    """eval mode: BatchNorm(conv_nobias + conv_bias) = conv_nobias scale + shift -> (scale, T), (shift, T)"""
    scale = gamma / torch.sqrt(rv + EPS)
    cb = conv_bias if conv_bias is not None else torch.zeros_like(rm)
    return (scale, scale.abs()), (beta + (cb - rm) * scale, beta.abs() + (cb.abs() + rm.abs()) * scale.abs())


def _windows(t):
    """(N, H, W, C) -> (N, H / 2, W / 2, C, 4): the 2 x 2 windows, row-major inside"""
    N, H, W, Cc = t.shape
    return t.reshape(N, H // 2, 2, W // 2, 2, Cc).permute(0, 1, 3, 5, 2, 4).reshape(N, H // 2, W // 2, Cc, 4)


def _unwindows(w):
    N, Ho, Wo, Cc, _ = w.shape
    return w.reshape(N, Ho, Wo, Cc, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(N, 2 * Ho, 2 * Wo, Cc)


def ref_bn_act_pool(x, sc, sh, pool):
    """x (N, H, W, C) fp64 -> [MaxPool2d(2)](ReLU(x sc + sh)) (sc, sh None: of x itself), and T = |x sc| + |sh| (its maximum over the window:
    the maximum of rounded values is within the largest single error of the maximum)"""
    v = x if sc is None else x * sc + sh
    T = x.abs() if sc is None else (x * sc).abs() + sh.abs()
    v = torch.relu(v)
    if pool:
        v, T = _windows(v).amax(-1), _windows(T.expand_as(x)).amax(-1)
    return v, T.expand_as(v)


def ref_bn_dv(x, dy, sc, sh, pool, last_max=False):
    """d v of v = x sc + sh behind ReLU (+ MaxPool2d(2)): dy where v > 0; pooled: at the FIRST maximum of the window in row-major order (as
    torch), nothing where the whole window is <= 0"""
    r = torch.relu(x * sc + sh)
    if not pool:
        return torch.where(r > 0, dy, torch.zeros_like(dy))
    w = _windows(r)
    arg = 3 - w.flip(-1).argmax(-1) if last_max else w.argmax(-1)
    sel = F.one_hot(arg, 4).to(D) * (w.amax(-1) > 0).to(D).unsqueeze(-1) * dy.unsqueeze(-1)
    return _unwindows(sel)


def ref_bn_bwd(x, dy, mean, istd, sc, sh, gamma, pool, last_max=False):
    """the BatchNorm (train) + ReLU (+ pool) backward -> name -> (value, T): dx = gamma istd (dv - s1 / n - xhat s2 / n), dbeta = s1 = sum dv,
    dgamma = s2 = sum dv xhat, xhat = (x - mean) istd"""
    dv = ref_bn_dv(x, dy, sc, sh, pool, last_max)
    n = x.shape[0] * x.shape[1] * x.shape[2]
    xh = (x - mean) * istd
    s1, s2 = dv.sum((0, 1, 2)), (dv * xh).sum((0, 1, 2))
    k = gamma * istd
    return dict(dx=(k * (dv - s1 / n - xh * s2 / n), k.abs() * (dv.abs() + s1.abs() / n + xh.abs() * s2.abs() / n)),
                dbeta=(s1, dv.abs().sum((0, 1, 2))), dgamma=(s2, (dv * xh).abs().sum((0, 1, 2))))


def ref_conv_bn_relu(x, w, scale, shift):
    """x (M, H, W, cin), w (cout, cin, 3, 3) fp64 -> ReLU(conv(x) scale + shift) (M, cout, H, W), T = |scale| sum |terms| + |shift|"""
    z, s, b = _nchw(x), scale.view(1, -1, 1, 1), shift.view(1, -1, 1, 1)
    return torch.relu(F.conv2d(z, w, None, padding=1) * s + b), F.conv2d(z.abs(), w.abs(), None, padding=1) * s.abs() + b.abs()


def ref_stem_dgrad(g, w, step=4096):
    """g (M, H, W, 64), w (64, 2, 3, 3) fp64 -> d in (M, 2, H, W) of conv2d(in, w, padding=1), and T; in chunks of images"""
    out, T = [], []
    for m0 in range(0, g.shape[0], step):
        z = _nchw(g[m0:m0 + step].to(D))
        out.append(F.conv_transpose2d(z, w, padding=1))
        T.append(F.conv_transpose2d(z.abs(), w.abs(), padding=1))
    return torch.cat(out), torch.cat(T)


def ref_fc_to_ref(y, mask, keep=2.0, hwc=False):
    """y (B, 256, 128) NHWC -> fc1's input (B, 32768) in the reference's (C, H, W) flatten order k = c 256 + hw, times the train-mode dropout
    `mask` (B, 32768, in that order; None: eval) with the kept activations scaled by 1 / (1 - p) = 2"""
    xr = y.reshape(y.shape[0], FCK) if hwc else y.permute(0, 2, 1).reshape(y.shape[0], FCK)
    return xr if mask is None else xr * mask.to(D) * keep


def ref_fc_from_ref(dxr, mask):
    """dxr (B, 32768) -> d y (B, 256, 128)"""
    g = dxr if mask is None else dxr * mask.to(D) * 2.0
    return g.reshape(-1, 128, 256).permute(0, 2, 1)


def ref_fc1(xr, w, b, block=128, shift_group=False):
    """xr (B, 32768) fp64, w (1024, 32768) f32 (taken in blocks of rows), b (1024) -> ReLU(b + xr w^T) (B, 1024), and T"""
    if shift_group:         # the wrong reference: samples 32.. read from the group in front of theirs
        xr = torch.cat([xr[:32], xr[:xr.shape[0] - 32]])
    y = torch.empty((xr.shape[0], w.shape[0]), dtype=D)
    T = torch.empty_like(y)
    for j0 in range(0, w.shape[0], block):
        wb = w[j0:j0 + block].to(D)
        y[:, j0:j0 + block], T[:, j0:j0 + block] = xr @ wb.T, xr.abs() @ wb.abs().T
    return torch.relu(y + b), T + b.abs()


def ref_fc1_bwd_w(dz1, xr, j0, j1):
    """rows j0..j1 of d fc1.weight = dz1^T xr, and T"""
    a = dz1[:, j0:j1].T
    return a @ xr, a.abs() @ xr.abs()


def ref_fc1_bwd_x(dz1, w, block=128):
    """dxr (B, 32768) = dz1 w, w (J, 32768) f32 taken in blocks of rows, and T"""
    want, T = torch.zeros((dz1.shape[0], w.shape[1]), dtype=D), torch.zeros((dz1.shape[0], w.shape[1]), dtype=D)
    for j0 in range(0, w.shape[0], block):
        wb = w[j0:j0 + block].to(D)
        want += dz1[:, j0:j0 + block] @ wb
        T += dz1[:, j0:j0 + block].abs() @ wb.abs()
    return want, T


def ref_fc2(y, w2):
    return y @ w2.T, y.abs() @ w2.abs().T


def ref_fc2_bwd(dtheta, y1, w2, gate_ge=False):
    """theta = ReLU-output y1 (B, 1024) times w2^T (2, 1024) -> name -> (value, T): dz1 = (y1 > 0) dtheta w2, dw2 = dtheta^T y1, db1 = sum_b dz1"""
    gate = (y1 >= 0 if gate_ge else y1 > 0).to(D)
    dz, Tz = gate * (dtheta @ w2), gate * (dtheta.abs() @ w2.abs())
    return dict(dz1=(dz, Tz), dw2=(dtheta.T @ y1, dtheta.abs().T @ y1.abs()), db1=(dz.sum(0), Tz.sum(0)))


def ref_adam(p, g, m, v, lr, b1, b2, eps, wd, step, m_new=None, v_new=None, no_bc2=False, eps_inside=False):
    """torch.optim.Adam's step (no amsgrad) in fp64 -> m', T_m, v', T_v, p', |update|; p' from (m_new, v_new) when given"""
    gj, ga = g + wd * p, g.abs() + wd * p.abs()
    m1, Tm = b1 * m + (1 - b1) * gj, b1 * m.abs() + (1 - b1) * ga
    v1, Tv = b2 * v + (1 - b2) * gj * gj, b2 * v.abs() + (1 - b2) * ga * ga
    mm, vv = (m1, v1) if m_new is None else (m_new, v_new)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 if no_bc2 else 1.0 - b2 ** step
    denom = torch.sqrt(vv / bc2 + eps) if eps_inside else torch.sqrt(vv) / np.sqrt(bc2) + eps
    upd = (lr / bc1) * mm / denom
    return m1, Tm, v1, Tv, p - upd, upd.abs()


BN_NPIX = {"256": 256, "257": 257, "255x256+1": 255 * 256 + 1, "147456": 147456}
HIGH = {F32: 1e8, BF16: 1e4}         # mean^2 / var of the worst channel (bf16's 8 bits hold no more than 4 x 256^2)


def bn_stats_inputs(npix, Cc, dt, seed):
    """x (npix, C) in dt: ordinary channels; channel 3 (f32: 4 too) a large mean with a small spread, mean^2 / var >= HIGH[dt] (bf16: 100 +-
    one ulp, which survives the rounding); channels 5, 6, 7 exactly constant (0, 0.37, -3.25).  gamma of both signs."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((npix, Cc), generator=g) * 0.7 + torch.linspace(-1, 1, Cc)
    if dt == BF16:
        x[:, 3] = 100.0 + 0.5 * torch.randint(-1, 2, (npix,), generator=g).float()
    else:
        x[:, 3] = 100.0 + 0.008 * torch.randn(npix, generator=g)
        x[:, 4] = -1000.0 + 0.08 * torch.randn(npix, generator=g)
    x[:, 5], x[:, 6], x[:, 7] = 0.0, 0.37, -3.25
    if dt == BF16:
        x = x.to(torch.bfloat16).float()
    gamma = torch.rand(Cc, generator=g) + 0.5
    gamma[1::2] *= -1
    return x, gamma, torch.randn(Cc, generator=g) * 0.1, torch.randn(Cc, generator=g) * 0.1, torch.rand(Cc, generator=g) + 0.5


def _window_counts(v):
    """(tied windows, windows that are all <= 0) of the pre-pool activation v (N, H, W, C), already through ReLU"""
    w = _windows(v)
    top = w.amax(-1, keepdim=True)
    return int((((w == top).sum(-1) > 1) & (top[..., 0] > 0)).sum()), int((top[..., 0] <= 0).sum())


def _stem_dgrad_w(seed):
    return (torch.randn((64, 2, 3, 3), generator=torch.Generator().manual_seed(seed)) * 0.2).to(torch.bfloat16).float()


def _mask(B, seed):
    return (torch.rand((B, FCK), generator=torch.Generator().manual_seed(seed)) >= 0.5).to(torch.uint8)


FC1_NSEQ = 16 * 64 + 32 + 1          # per wave 16 stages x 64 k on one accumulator, then 32 slabs and the bias in fc1_finish_kernel
FCX_NSEQ = 256 + 3                   # per wave 128 steps x 2 j on one accumulator, then the four waves' sums


ADAM_SETTINGS = [(1e-3, 0.9, 0.999, 0.0, 1), (3e-3, 0.9, 0.99, 1e-2, 2), (1e-4, 0.9, 0.999, 0.0, 1000)]     # lr, beta1, beta2, wd, step
ADAM_EPS = 1e-8


def adam_inputs(n, seed):
    """p, g, m, v (>= 0) fp32, with elements of g = 0, v = 0, m = 0 and g = 1e-30 (g^2 underflows)"""
    gen = torch.Generator().manual_seed(seed)
    p, g, m = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.1, torch.randn(n, generator=gen) * 0.05
    v = torch.rand(n, generator=gen) * 0.01
    g[4::7], v[5::11], m[6::13], g[7::17] = 0.0, 0.0, 0.0, 1e-30
    return p, g, m, v


def _adam_p_ratio(r, **wrong):
    """p' against the fp64 formula on the m', v' the kernel stored: 2^-24 max(|got|, |want|) + C |update|"""
    _, _, _, _, want, upd = ref_adam(*r["ins"], *r["hyper"], m_new=r["m"], v_new=r["v"], **wrong)
    return (r["p"] - want).abs() / (2.0 ** -24 * torch.maximum(r["p"].abs(), want.abs()) + C * upd + 1e-300)


# ----------------------------------------------------------------------------------------------------------- the registered tail
# The Lanczos shift and its backward (csrc/lanczos.hip, lanczos_bwd.hip) and the loss / score kernels (csrc/losses.hip): the definitions in
# fp64, the inputs, the cases and the checks that tests/test_gpu_kernels_tail.py runs on the GPU's outputs and
# tests/test_kernels_tail_host.py on a float32 restatement's.  A `k` below is either of the two: an object whose methods taps, shift,
# shift_bwd, get_loss, loss_train, loss_bwd and shift_cpsnr take CPU float32 tensors and return what the kernels wrote, on the CPU.
from kernel_bounds import C_TAIL, U32, U64, _assert_close, _assert_within, _ratio, _within_ratio, cmse_bound, cpsnr_bound   # noqa: E402

D64 = torch.float64
PI32 = float(np.float32(np.pi))             # the kernels' pi: float32(pi), here widened to fp64


def _tap_t(d, freeze="where"):
    """t = pi ((j - 3) - d), (n, 7), and the mask of the taps held constant.  freeze: "where" - the definition: t == 0 is replaced by 1e-6
    through a where, so that tap passes no gradient; "live" - 1e-6 is added instead, the tap keeps its gradient; "centre" - the wrong
    variant that holds the centre tap j = 3 constant instead of the t == 0 tap"""
    j = torch.arange(7, dtype=D64) - 3
    t = PI32 * (j[None, :] - d.reshape(-1, 1))
    hit = t == 0
    if freeze == "where":
        return torch.where(hit, torch.full_like(t, 1e-6), t), hit
    t = t + 1e-6 * hit
    if freeze == "live":
        return t, torch.zeros_like(hit)
    centre = (j == 0)[None, :].expand_as(t)
    return torch.where(centre, t.detach(), t), centre


def ref_taps(d, freeze="where"):
    """d (n,) fp64 -> k (n, 7) = u / sum u, u = sinc(t) sinc(t / 3), and T_j = (1 + 7 |k_j|) / |sum u|: t is rounded to fp32 before the sine,
    so every u_j carries an ABSOLUTE error e of order 2^-24, and k_j = u_j / s one of (e + |k_j| 7 e) / |s|"""
    t, _ = _tap_t(d, freeze)
    u = torch.sin(t) / t * (torch.sin(t / 3) / (t / 3))
    s = u.sum(1, keepdim=True)
    k = u / s
    return k, ((1 + 7 * k.abs()) / s.abs()).detach()


def ref_tap_grad(d):
    """d (n,) fp64 -> dk_j / dd (n, 7) in closed form (the host test holds it to autograd's) and T of it.  With A = sinc t, B = sinc t/3:
    du = -pi (A' B + A B'), A' = (t cos t - sin t) / t^2, 0 for a frozen tap.  t is rounded to fp32 before the sine and the cosine, so
    each of A, B, A', B' carries an absolute error e of the order of one rounding besides its relative ones, T(A) = |A| + 1 and
    T(A') = Ta' + 1 with Ta' = A' on absolute values (that difference cancels for small |t|: T is large, the bound loose, at a shift
    close to but not on an integer); T_du = pi [2 Ta' |B| + |B| + Ta' + 2 |A| Tb' + |A| + Tb'].  dk = du / s - k ds / s, whose error with
    e on every u, 7 e on s, e T_j on k is
      e [ T_du / |s| + 7 |du| / s^2 + T_j |ds| / |s| + |k| sum T_du / |s| + 7 |k| |ds| / s^2 + 2 (|du| / |s| + |k| |ds| / |s|) ]
    (the last term: the roundings of (du s - u ds) / s^2 itself)"""
    t, hit = _tap_t(d.detach())
    t3 = t / 3
    A, B = torch.sin(t) / t, torch.sin(t3) / t3
    dA, dB = (torch.cos(t) * t - torch.sin(t)) / t ** 2, (torch.cos(t3) * t3 - torch.sin(t3)) / t3 ** 2 / 3
    dAa = (torch.cos(t).abs() * t.abs() + torch.sin(t).abs()) / t ** 2
    dBa = (torch.cos(t3).abs() * t3.abs() + torch.sin(t3).abs()) / t3 ** 2 / 3
    zero = torch.zeros_like(t)
    du = torch.where(hit, zero, -PI32 * (dA * B + A * dB))
    dua = torch.where(hit, zero, PI32 * (2 * dAa * B.abs() + B.abs() + dAa + 2 * A.abs() * dBa + A.abs() + dBa))
    u = A * B
    s, ds = u.sum(1, keepdim=True), du.sum(1, keepdim=True)
    k, sa = u / s, s.abs()
    Tj = (1 + 7 * k.abs()) / sa
    Tdk = (dua / sa + 7 * du.abs() / s ** 2 + Tj * ds.abs() / sa + k.abs() * dua.sum(1, keepdim=True) / sa + 7 * k.abs() * ds.abs() / s ** 2
           + 2 * (du.abs() / sa + k.abs() * ds.abs() / sa))
    return (du * s - u * ds) / s ** 2, Tdk


def shift_with_taps(img, ky, kx, edge="reflect"):
    """P = pad-3(img) (reflection without edge repeat); out[y][x] = sum_n kx[n] sum_m ky[m] P[y + m][x + n]: vertical, then horizontal.
    img (b, c, H, W), ky / kx (b, c, 7).  edge = "replicate": the wrong border"""
    H, W = img.shape[2:]
    P = F.pad(img, (3, 3, 3, 3), mode=edge)
    V = sum(ky[:, :, m, None, None] * P[:, :, m:m + H, :] for m in range(7))
    return sum(kx[:, :, n, None, None] * V[:, :, :, n:n + W] for n in range(7))


def _plane_rows(b, c, by_plane=False):
    """the row of `shift` each plane (b, c) takes: plane % C; by_plane: the plane's running number instead (folded into the table)"""
    p = torch.arange(b * c)
    return (p // b if by_plane else p % c).reshape(b, c)


def ref_lanczos_shift(img, shift, edge="reflect", swap=False, by_plane=False, freeze="where"):
    """img (b, c, H, W), shift (c, 2) = (dy, dx) per channel, fp64 torch: d_img and d_shift come from autograd.  swap (dy and dx exchanged),
    by_plane, edge and freeze are the negative controls"""
    b, c = img.shape[:2]
    sh = shift.flip(1) if swap else shift
    rows = _plane_rows(b, c, by_plane)
    return shift_with_taps(img, ref_taps(sh[:, 0], freeze)[0][rows], ref_taps(sh[:, 1], freeze)[0][rows], edge)


def ref_lanczos_grads(img, shift, dout, **wrong):
    img, shift = img.clone().requires_grad_(True), shift.clone().requires_grad_(True)
    (ref_lanczos_shift(img, shift, **wrong) * dout).sum().backward()
    return img.grad, shift.grad


def _abs_taps(shift, b):
    """per axis (|k|, |k| + e), e = C_TAIL T_j the tap's own error, each (b, c, 7)"""
    out = []
    for ax in (0, 1):
        k, Tj = ref_taps(shift[:, ax].detach())
        out.append((k.abs()[None].expand(b, -1, -1), (k.abs() + C_TAIL * Tj)[None].expand(b, -1, -1)))
    return out


def _with_tap_error(base, full):
    """T with C_TAIL T = C_TAIL base + (full - base): the fp32 roundings of the sum on exact taps, plus what the taps' errors e move it by;
    base = sum |ky| |kx| |P|, full = sum (|ky| + e_y)(|kx| + e_x) |P|"""
    return base + (full - base) / C_TAIL


def lanczos_shift_T(img, shift):
    (ya, yi), (xa, xi) = _abs_taps(shift, img.shape[0])
    return _with_tap_error(shift_with_taps(img.abs(), ya, xa), shift_with_taps(img.abs(), yi, xi))


def _adjoint(dout, ky, kx):
    x = torch.zeros_like(dout, requires_grad=True)
    return torch.autograd.grad(shift_with_taps(x, ky, kx), x, dout)[0]


def lanczos_dimg_T(dout, shift):
    """the same with |dout|, folded back through the reflection"""
    (ya, yi), (xa, xi) = _abs_taps(shift, dout.shape[0])
    return _with_tap_error(_adjoint(dout.abs(), ya, xa), _adjoint(dout.abs(), yi, xi))


def tap_sums(img, dout, ky, kx):
    """G (c, 2, 7): dL / dky[m] = sum dout[y][x] HP[y + m][x], HP = the horizontal pass of the padded rows; dL / dkx[n] = sum dout[y][x]
    V[y][x + n], V = the vertical pass; summed over the batch"""
    H, W = img.shape[2:]
    P = F.pad(img, (3, 3, 3, 3), mode="reflect")
    HP = sum(kx[:, :, n, None, None] * P[:, :, :, n:n + W] for n in range(7))
    V = sum(ky[:, :, m, None, None] * P[:, :, m:m + H, :] for m in range(7))
    Gy = torch.stack([(dout * HP[:, :, m:m + H]).sum((0, 2, 3)) for m in range(7)], 1)
    Gx = torch.stack([(dout * V[:, :, :, n:n + W]).sum((0, 2, 3)) for n in range(7)], 1)
    return torch.stack([Gy, Gx], 1)


def lanczos_dshift_T(img, shift, dout):
    """d shift = sum_j dk_j G_j: T = sum_j |dk_j| T(G_j) + T(dk_j) sum |dout| |HP|, T(G_j) = sum |dout| |HP| with the taps' error as above"""
    (ya, yi), (xa, xi) = _abs_taps(shift, img.shape[0])
    Gb, Gf = tap_sums(img.abs(), dout.abs(), ya, xa), tap_sums(img.abs(), dout.abs(), yi, xi)
    T = torch.zeros((shift.shape[0], 2), dtype=D64)
    for ax in (0, 1):
        dk, Tdk = ref_tap_grad(shift[:, ax])
        T[:, ax] = (dk.abs() * _with_tap_error(Gb[:, ax], Gf[:, ax]) + Tdk * Gb[:, ax]).sum(1)
    return T


# shifts: dy != dx in every channel; channel 0 an integer shift on the rows only (the frozen tap off-centre: j = 5), channel 1 beyond the
# +-3 support on the rows, channel 2 an integer shift on the columns only.  c = 1 takes one of the rows, by the shape.
TAIL_SHIFTS = torch.tensor([[2.0, -0.63], [-3.5, 0.5], [0.37, -1.0]])
LANCZOS_BC = [(1, 1), (2, 3)]
LANCZOS_FWD_SHAPES = [(4, 4), (4, 135), (5, 7), (32, 128), (33, 129), (38, 134), (70, 20)]      # the forward's tile: 32 x 128
LANCZOS_BWD_SHAPES = [(4, 4), (5, 64), (16, 64), (17, 65), (7, 9)]                              # the backward's tile: 16 x 64
TAP_N = [1, 63, 64, 65]
TAP_D = ([0.0, -0.0] + [s * v for v in (1.0, 2.0, 3.0) for s in (1, -1)]
         + [i + s * e for i in (0.0, 1.0, -2.0, 3.0) for e in (1e-6, 1e-4) for s in (1, -1)]
         + [0.5, -0.5, 2.999, -2.999, 3.5, -7.25])


def tap_inputs(n):
    """n shifts out of TAP_D, from a start that moves with n (n >= 63 takes every one)"""
    return torch.tensor([TAP_D[(n + i) % len(TAP_D)] for i in range(n)], dtype=torch.float32)


def lanczos_inputs(b, c, H, W):
    """img (values around 0.5: a DC offset), shift, dout, and the values d_shift starts from: float32"""
    g = torch.Generator().manual_seed(7000 + 131 * H + 7 * W + b)
    img = 0.5 + 0.25 * torch.randn((b, c, H, W), generator=g)
    dout = torch.randn((b, c, H, W), generator=g)
    shift = TAIL_SHIFTS.clone() if c == 3 else TAIL_SHIFTS[(H + W) % 3][None].clone()
    return img, shift, dout, torch.randn((c, 2), generator=g)


def check_taps(k, n):
    d = tap_inputs(n)
    want, T = ref_taps(d.double())
    return _assert_close(f"taps n={n}", "f32", k.taps(d), want, T, layout="i j", c=C_TAIL)


def check_lanczos_fwd(k, b, c, H, W):
    img, shift, _, _ = lanczos_inputs(b, c, H, W)
    tag = f"lanczos_shift b={b} c={c} {H}x{W}"
    r = _assert_close(tag, "f32", k.shift(img, shift), ref_lanczos_shift(img.double(), shift.double()), lanczos_shift_T(img.double(), shift.double()),
                      layout="b c y x", c=C_TAIL)
    if b > 1:                                           # the same image in every batch entry: the same planes (plane % C picks the shift)
        img[1:] = img[:1]
        same = k.shift(img, shift)
        assert all(torch.equal(same[i], same[0]) for i in range(1, b)), f"{tag}: equal images, different planes"
    return r


def check_lanczos_bwd(k, b, c, H, W):
    """d_img, d_shift (+= into non-zero values) against autograd of the where form - at the integer shifts that is the frozen tap's
    gradient, exactly none; then each output alone, the other one NULL: bit-identical"""
    img, shift, dout, start = lanczos_inputs(b, c, H, W)
    tag = f"lanczos_shift_backward b={b} c={c} {H}x{W}"
    d_img, d_shift = k.shift_bwd(img, shift, dout, start)
    i64, s64, o64 = img.double(), shift.double(), dout.double()
    wi, ws = ref_lanczos_grads(i64, s64, o64)
    r1 = _assert_close(tag + " d_img", "f32", d_img, wi, lanczos_dimg_T(o64, s64), layout="b c y x", c=C_TAIL)
    r2 = _assert_close(tag + " d_shift", "f32", d_shift, start.double() + ws, start.double().abs() + lanczos_dshift_T(i64, s64, o64), layout="c axis", c=C_TAIL)
    none, only_shift = k.shift_bwd(img, shift, dout, start, need_img=False)
    assert none is None and torch.equal(only_shift, d_shift), f"{tag}: d_shift changes when d_img is NULL"
    only_img, none = k.shift_bwd(img, shift, dout, None)
    assert none is None and torch.equal(only_img, d_img), f"{tag}: d_img changes when d_shift is NULL"
    return max(r1, r2)


# ---- losses and the score
def crop_mask(S, crop):
    """get_crop_mask: ones, a border of `crop` pixels zero (crop = 0: no border)"""
    m = torch.ones((S, S), dtype=D64)
    if crop > 0:
        m[:crop], m[-crop:], m[:, :crop], m[:, -crop:] = 0, 0, 0, 0
    return m


def ref_losses(srs, hrs, maps, crop, square_mask=False, drop=None):
    """train.get_loss on the cropped map, (B, S, S) fp64, in its own two passes: n = sum m, the brightness bias b = sum m (hr - sr) / n,
    cMSE = sum m (sr + b - hr)^2 / n (the weight is m, not m^2), cPSNR = -10 log10 cMSE, masked_MSE = mean (m sr - m hr)^2; and the bounds
    of the kernels' fp64 sums.  square_mask (m^2 as the weight) and drop (one pixel left out) are the negative controls"""
    S = srs.shape[-1]
    m = maps * crop_mask(S, crop)
    if drop is not None:
        m = m.clone()
        m[drop] = 0
    d = srs - hrs
    S0, S1, S2 = m.sum((1, 2)), (m * d).sum((1, 2)), (m * d * d).sum((1, 2))
    bias = (m * (hrs - srs)).sum((1, 2)) / S0
    cmse = ((m * m if square_mask else m) * (srs + bias[:, None, None] - hrs) ** 2).sum((1, 2)) / S0
    mmse = ((m * srs - m * hrs) ** 2).mean((1, 2))
    e = cmse_bound(S * S, S0, S1, S2)
    return dict(m=m, S0=S0, bias=bias, cmse=cmse, cpsnr=-10 * torch.log10(cmse), mmse=mmse, e_S0=S * S * U64 * S0,
                e_bias=S * S * U64 * (m * d.abs()).sum((1, 2)) / S0, e_cmse=e, e_cpsnr=cpsnr_bound(cmse, e), e_mmse=S * S * U64 * mmse)


def ref_loss_grad(srs, hrs, r, metric, d_out):
    """d_srs = d_out (d out / d cMSE) 2 m (d + b) / n, the bias a constant (train.py detaches it); T = |coef| m (|sr| + |hr| + |b|)"""
    dm = torch.ones_like(r["cmse"]) if metric == 1 else -10.0 / (np.log(10.0) * r["cmse"])
    coef = (d_out * dm * 2 / r["S0"])[:, None, None]
    b = r["bias"][:, None, None]
    return coef * r["m"] * (srs - hrs + b), coef.abs() * r["m"] * (srs.abs() + hrs.abs() + b.abs())


LOSS_S = [1, 3, 16, 17, 65]
TRAIN_S = [3, 17, 65, 129]          # fewer pixels than the 16 slices; a ragged last slice; 65; 16 641 pixels > the backward's 64 x 256 grid


def crops(S):
    return sorted({cr for cr in (0, 3, (S - 1) // 2) if 2 * cr < S})


def loss_inputs(B, S, kind, ill=False):
    """srs, hrs, maps float32.  kind: "bin" (0 / 1), "frac" (values in [0, 1], a fifth exact zeros), "zero" (sample 0 all zero, the others
    binary), "mixed" (binary and fractional samples in turn).  The centre pixel of every map that is not all zero is 1, so a crop never
    leaves a sample without a clear pixel.  ill: sr = hr + 0.2 + 1e-3 noise, S2 ~ S1^2 / S0"""
    g = torch.Generator().manual_seed(9000 + 17 * S + B + 1000 * ["bin", "frac", "zero", "mixed"].index(kind) + (5 if ill else 0))
    hrs = 0.1 + 0.6 * torch.rand((B, S, S), generator=g)
    noise = torch.randn((B, S, S), generator=g)
    srs = hrs + 0.2 + 1e-3 * noise if ill else hrs + 0.02 + 0.05 * noise
    binary = (torch.rand((B, S, S), generator=g) > 0.3).float()
    frac = torch.rand((B, S, S), generator=g) * (torch.rand((B, S, S), generator=g) > 0.2)
    if kind == "frac":
        maps = frac
    elif kind == "mixed":
        maps = torch.where((torch.arange(B) % 2 == 0)[:, None, None], binary, frac)
    else:
        maps = binary
    maps[:, S // 2, S // 2] = 1.0
    if kind == "zero":
        maps[0] = 0.0
    return srs, hrs, maps


def check_get_loss(k, S, crop, B, kind, ill=False):
    srs, hrs, maps = loss_inputs(B, S, kind, ill)
    r = ref_losses(srs.double(), hrs.double(), maps.double(), crop)
    tag = f"get_loss S={S} crop={crop} B={B} {kind}{' ill' if ill else ''}"
    worst = 0.0
    for metric, key in ((0, "mmse"), (1, "cmse"), (2, "cpsnr")):
        want = r[key]
        worst = max(worst, _assert_within(f"{tag} metric {metric}", k.get_loss(srs, hrs, maps, crop, metric), want, r["e_" + key] + U32 * want.abs(), "b"))
    return worst


def train_d_out(B):
    """different per sample, with a zero and a negative one (B = 1: negative)"""
    d = torch.randn(B, generator=torch.Generator().manual_seed(77 + B)) + 0.25
    d[0] = -0.75
    if B > 2:
        d[1], d[2] = 0.0, -1.5
    return d


def check_loss_train(k, S, crop, B, kind, metric, drop=None):
    """loss_partial + loss_finish: out and stats = (S0, -S1 / S0, cMSE, 0); loss_backward_kernel on those stats: d_srs, exact zeros where
    the cropped map is zero.  Where cMSE lies within rounding of zero (a one-pixel window) cPSNR and its gradient are not determined, and
    only the stats are checked."""
    srs, hrs, maps = loss_inputs(B, S, kind)
    s64, h64 = srs.double(), hrs.double()
    r = ref_losses(s64, h64, maps.double(), crop, drop=drop)
    tag = f"get_loss_train S={S} crop={crop} B={B} {kind} metric {metric}"
    out, stats = k.loss_train(srs, hrs, maps, crop, metric)
    worst = _assert_within(tag + " S0", stats[:, 0], r["S0"], r["e_S0"], "b")
    worst = max(worst, _assert_within(tag + " bias", stats[:, 1], r["bias"], r["e_bias"], "b"))
    worst = max(worst, _assert_within(tag + " cMSE", stats[:, 2], r["cmse"], r["e_cmse"], "b"))
    assert bool((stats[:, 3] == 0).all()) and not bool(torch.signbit(stats[:, 3]).any()), f"{tag}: the fourth word of stats is not 0"
    want = r["cmse"] if metric == 1 else r["cpsnr"]
    e = r["e_cmse"] if metric == 1 else r["e_cpsnr"]
    worst = max(worst, _assert_within(tag + " out", out, want, e + U32 * want.abs(), "b"))
    d_out = train_d_out(B)
    d_srs = k.loss_bwd(srs, hrs, maps, stats, d_out, crop, metric)
    det = torch.isfinite(e)
    assert bool(det.any()) or S - 2 * crop == 1, f"{tag}: no sample with a determined gradient"
    if bool(det.any()):
        gw, T = ref_loss_grad(s64, h64, r, metric, d_out.double())
        worst_g = _assert_close(tag + " d_srs", "f32", d_srs[det], gw[det], T[det], layout="b y x", c=C_TAIL)
        off = r["m"][det] == 0
        assert bool((d_srs[det][off] == 0).all()), f"{tag}: d_srs is not 0 where the cropped map is"
        assert bool(off.any()) or crop == 0
        assert bool((d_srs[det][d_out[det] == 0] == 0).all())
        return worst, worst_g
    return worst, 0.0


SCORE_BORDERS = [0, 1, 3]
PLANTED = {0: (0, 0), 1: (1, -1), 3: (1, -2)}       # (rows, columns): unequal, so a transposed offset scores visibly worse


def score_inputs(B, S, border):
    """hrs in [0.1, 0.9]; srs = hrs moved by PLANTED[border] + noise + a brightness offset, with values below 0 and above 1; binary maps"""
    g = torch.Generator().manual_seed(12000 + 31 * S + 7 * border + B)
    hrs = 0.1 + 0.8 * torch.rand((B, S, S), generator=g)
    pu, pv = PLANTED[border]
    srs = torch.roll(hrs, (-pu, -pv), (1, 2)) + 0.003 + 0.01 * torch.randn((B, S, S), generator=g)
    sel = torch.rand((B, S, S), generator=g)
    srs = torch.where(sel < 0.03, torch.full_like(srs, -0.2), torch.where(sel > 0.97, torch.full_like(srs, 1.3), srs))
    return srs, hrs, (torch.rand((B, S, S), generator=g) > 0.1).float()


def ref_shift_scores(srs, hrs, maps, border, clip, transpose=False):
    """Evaluator.shift_cPSNR's per-offset cPSNR, (B, (2 border + 1)^2) at k = u (2 border + 1) + v for the row offset u and the column offset
    v of hr and its map against the centre crop of sr (np.clip first when clip: NaN stays NaN), on BINARY maps; and each score's bound.
    bias = sum (hr - sr) m / n, cMSE = sum ((hr - sr - bias) m)^2 / n, n = sum m.  transpose: (u, v) exchanged, the negative control"""
    B, S, _ = srs.shape
    size, nb = S - 2 * border, 2 * border + 1
    s = srs[:, border:border + size, border:border + size]
    if clip:
        s = s.clamp(0, 1)
    scores, bounds = torch.zeros((B, nb * nb), dtype=D64), torch.zeros((B, nb * nb), dtype=D64)
    for u in range(nb):
        for v in range(nb):
            uu, vv = (v, u) if transpose else (u, v)
            hr, m = hrs[:, uu:uu + size, vv:vv + size], maps[:, uu:uu + size, vv:vv + size]
            n, diff = m.sum((1, 2)), hr - s
            bias = (diff * m).sum((1, 2)) / n
            cmse = (((diff - bias[:, None, None]) * m) ** 2).sum((1, 2)) / n
            scores[:, u * nb + v] = -10 * torch.log10(cmse)
            bounds[:, u * nb + v] = cpsnr_bound(cmse, cmse_bound(size * size, n, (m * diff).sum((1, 2)), (m * diff * diff).sum((1, 2))))
    return scores, bounds


def ref_score_max(scores, bounds):
    """np.max over the offsets (a NaN score makes it NaN) as the float the kernel stores, and its bound"""
    want = torch.where(torch.isnan(scores).any(1), torch.full((scores.shape[0],), float("nan"), dtype=D64), scores.amax(1))
    return want, torch.where(torch.isnan(bounds), torch.zeros_like(bounds), bounds).amax(1) + U32 * want.abs()


def check_shift_cpsnr(k, border, S, B, clip):
    srs, hrs, maps = score_inputs(B, S, border)
    tag = f"shift_cpsnr border={border} S={S} B={B} clip={clip}"
    scores, out = k.shift_cpsnr(srs, hrs, maps, border, clip)
    want, bounds = ref_shift_scores(srs.double(), hrs.double(), maps.double(), border, clip)
    worst = _assert_within(tag + " scores", scores, want, bounds, "b k")
    return max(worst, _assert_within(tag + " max", out, *ref_score_max(want, bounds), "b"))


# ---- negative controls: a reference wrong in one way must exceed the bound on the outputs that pass against the right one
TAIL_CONTROLS = ["edge_repeat", "dy_dx_swapped", "frozen_tap_centre", "shift_by_plane", "crop_off_by_one", "square_mask", "pixel_dropped",
                 "offsets_transposed"]


def tail_control(k, control):
    """-> (error / bound against the right reference, against the wrong one)"""
    if control in ("edge_repeat", "dy_dx_swapped", "shift_by_plane"):
        b, c, H, W = 2, 3, 5, 7
        img, shift, _, _ = lanczos_inputs(b, c, H, W)
        got, i64, s64 = k.shift(img, shift), img.double(), shift.double()
        T = lanczos_shift_T(i64, s64)
        wrong = {"edge_repeat": dict(edge="replicate"), "dy_dx_swapped": dict(swap=True), "shift_by_plane": dict(by_plane=True)}[control]
        return _ratio("f32", got, ref_lanczos_shift(i64, s64), T, C_TAIL)[0], _ratio("f32", got, ref_lanczos_shift(i64, s64, **wrong), T, C_TAIL)[0]
    if control == "frozen_tap_centre":
        b, c, H, W = 2, 3, 7, 9
        img, shift, dout, start = lanczos_inputs(b, c, H, W)
        _, got = k.shift_bwd(img, shift, dout, start, need_img=False)
        i64, s64, o64, st = img.double(), shift.double(), dout.double(), start.double()
        T = st.abs() + lanczos_dshift_T(i64, s64, o64)
        return (_ratio("f32", got, st + ref_lanczos_grads(i64, s64, o64)[1], T, C_TAIL)[0],
                _ratio("f32", got, st + ref_lanczos_grads(i64, s64, o64, freeze="centre")[1], T, C_TAIL)[0])
    if control in ("crop_off_by_one", "square_mask"):
        S, crop, B = 17, 3, 3
        srs, hrs, maps = loss_inputs(B, S, "frac")
        got = k.get_loss(srs, hrs, maps, crop, 1)
        r = ref_losses(srs.double(), hrs.double(), maps.double(), crop)
        bad = (ref_losses(srs.double(), hrs.double(), maps.double(), crop + 1) if control == "crop_off_by_one" else
               ref_losses(srs.double(), hrs.double(), maps.double(), crop, square_mask=True))
        return (_within_ratio(got, r["cmse"], r["e_cmse"] + U32 * r["cmse"].abs()),
                _within_ratio(got, bad["cmse"], bad["e_cmse"] + U32 * bad["cmse"].abs()))
    if control == "pixel_dropped":
        S, crop, B = 129, 3, 1
        srs, hrs, maps = loss_inputs(B, S, "bin")
        _, stats = k.loss_train(srs, hrs, maps, crop, 2)
        y, x = [int(v) for v in torch.nonzero(maps[0, crop:S - crop, crop:S - crop])[-1]]
        r = ref_losses(srs.double(), hrs.double(), maps.double(), crop)
        bad = ref_losses(srs.double(), hrs.double(), maps.double(), crop, drop=(0, y + crop, x + crop))
        return _within_ratio(stats[:, 2], r["cmse"], r["e_cmse"]), _within_ratio(stats[:, 2], bad["cmse"], bad["e_cmse"])
    assert control == "offsets_transposed", control
    srs, hrs, maps = score_inputs(1, 23, 3)
    scores, _ = k.shift_cpsnr(srs, hrs, maps, 3, 1)
    want, bounds = ref_shift_scores(srs.double(), hrs.double(), maps.double(), 3, 1)
    bad, bb = ref_shift_scores(srs.double(), hrs.double(), maps.double(), 3, 1, transpose=True)
    return _within_ratio(scores, want, bounds), _within_ratio(scores, bad, bb)
