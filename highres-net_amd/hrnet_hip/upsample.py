"""Bicubic x2 / x3 / x4 upsampling of float frames on device, with a gradient: the frame of HRNet's
`global_residual`, and ESA's baseline - "cPSNR of a bicubic upsample of an averaged clear frame" - for data without ESA's table
(`baseline`, `validate.baseline_table`).

`upsample` is one launch of `hrn_upsample` behind `torch.ops.hrnet_hip.upsample`, whose autograd formula is `hrn_upsample_backward`
(d_frames) and the identity (d_base).  The definition is that of torch.nn.functional.interpolate(mode="bicubic", align_corners=False)
with Keys' parameter `a` (include/hrnet_hip.h): an axis has only `scale` phases, so its scale x 4 tap weights are a table, computed here
on the host in fp64 and rounded to fp32 exactly as the library does before it hands them to the kernel - the device and a restatement
share their weights and differ in summation alone.  There is no CPU fallback: tensors must be on a ROCm device."""
import numpy as np
import torch

from . import binding
from .composite import masked_composite
from .resample import check_scale


def phase_weights(scale, a=-0.75):
    """-> (shift (scale,) int, weights (scale, 4) float32): output index j = scale * m + p reads the source indices
    m + shift[p] - 1 .. m + shift[p] + 2 (clamped to the axis) with weights[p]: w2(t + 1), w1(t), w1(1 - t), w2(2 - t) of
    t = x - floor(x), x = (p + 0.5) / scale - 0.5, w1(x) = ((a + 2) x - (a + 3)) x^2 + 1, w2(x) = ((a x - 5 a) x + 8 a) x - 4 a; fp64,
    rounded to fp32 (`a` itself goes through fp32 first, as it does through the C ABI)."""
    scale = check_scale(scale)
    a = float(np.float32(_check_a(a)))
    w1 = lambda x: ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    w2 = lambda x: ((a * x - 5.0 * a) * x + 8.0 * a) * x - 4.0 * a
    shift = np.zeros(scale, np.int64)
    weights = np.zeros((scale, 4), np.float64)
    for p in range(scale):
        x = (p + 0.5) / scale - 0.5
        i = int(np.floor(x))
        t = x - i
        shift[p] = i
        weights[p] = (w2(t + 1.0), w1(t), w1(1.0 - t), w2(2.0 - t))
    return shift, weights.astype(np.float32)


def _check_a(a):
    if isinstance(a, bool) or not isinstance(a, (int, float, np.floating, np.integer)):
        raise TypeError(f"a must be a number; got {a!r}")
    if not np.isfinite(a):
        raise ValueError(f"a must be finite; got {a!r}")
    return float(a)


def upsample(frames, scale, a=-0.75, base=None):
    """frames (..., H, W), base (..., scale H, scale W) or None -> base + up(frames), f32 (..., scale H, scale W): the leading dimensions
    are flattened to planes.  scale 2, 3 or 4; a: Keys' parameter (-0.75 torch / OpenCV, -0.5 Keys / Pillow); H, W in 1..16384.
    Differentiable in frames (the adjoint kernel) and in base (the identity)."""
    if not torch.is_tensor(frames):
        raise TypeError(f"frames must be a torch.Tensor; got {type(frames).__name__}")
    if base is not None and not torch.is_tensor(base):
        raise TypeError(f"base must be a torch.Tensor or None; got {type(base).__name__}")
    scale, a = check_scale(scale), _check_a(a)
    if not frames.is_floating_point() or (base is not None and not base.is_floating_point()):
        raise TypeError("frames and base must be floating-point tensors")
    if frames.dim() < 2 or frames.numel() == 0:
        raise ValueError(f"frames must be a non-empty (..., H, W); got {tuple(frames.shape)}")
    H, W = frames.shape[-2:]
    if max(H, W) > binding.UPSAMPLE_MAX_SIDE:
        raise ValueError(f"planes of 1..{binding.UPSAMPLE_MAX_SIDE} a side; got {H} x {W}")
    want = tuple(frames.shape[:-2]) + (scale * H, scale * W)
    if base is not None and tuple(base.shape) != want:
        raise ValueError(f"base must be {want} for frames {tuple(frames.shape)} at scale {scale}; got {tuple(base.shape)}")
    for name, t in (("frames", frames), ("base", base)):
        if t is not None and not t.is_cuda:
            raise TypeError(f"{name} is on '{t.device}': the upsampler runs on a ROCm device only (no CPU fallback)")
        if t is not None and t.device != frames.device:
            raise TypeError(f"{name} is on '{t.device}' but frames on '{frames.device}'")
    out = torch.ops.hrnet_hip.upsample(frames.reshape(-1, H, W), None if base is None else base.reshape(-1, scale * H, scale * W), scale, a)
    return out.view(want)


def baseline(lrs, alphas=None, lr_masks=None, scale=3, a=-0.75, n_ref=9):
    """lrs (B,V,H,W)[, alphas (B,V), lr_masks (B,V,H,W)] -> (B, 1, scale H, scale W): the bicubic upsample of the composite frame
    `masked_composite(lrs, lr_masks, alphas, n_ref)` - the median of the clear pixels of the first n_ref real views.  No gradient into
    lrs: the frame is data."""
    ref = masked_composite(lrs, lr_masks, alphas, n_ref=n_ref, fill=False)[0]
    return upsample(ref, scale, a).unsqueeze(1)
