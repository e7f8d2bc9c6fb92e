"""The fp64 references of the per-element kernel tests and the inputs they are evaluated at: each ref_* function restates in fp64, on the
exact values a kernel reads, what the kernel computes, and returns with it T = the same expression on absolute values.
tests/test_gpu_kernels_bwd.py and tests/test_gpu_kernels_shiftnet.py hold the kernels to them on the GPU; tests/test_kernels_bwd_host.py
and tests/test_kernels_shiftnet_host.py check the references themselves against torch autograd / torch.optim.Adam on the CPU, on the same
inputs and constants, which is why those live here too."""
import numpy as np
import torch
import torch.nn.functional as F

from kt import BF16, BF16X3, F32                        # noqa: F401
from kernel_bounds import BF, C, _nchw, rnd             # noqa: F401  (the host tests reach the conventions through this module)

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
    d = torch.nn.grad.conv2d_input((B * V, 2, H, W), w, _nchw(dA), padding=1).reshape(B, V, 2, H, W)
    Ta = torch.nn.grad.conv2d_input((B * V, 2, H, W), w.abs(), _nchw(dA).abs(), padding=1).reshape(B, V, 2, H, W)
    out, T = d[:, :, 0].clone(), Ta[:, :, 0].clone()
    sel = ref_route_index(lrs, ref, highest)[:, None]
    out.scatter_add_(1, sel, d[:, :, 1].sum(1, keepdim=True))
    T.scatter_add_(1, sel, Ta[:, :, 1].sum(1, keepdim=True))
    return out, T


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
