"""Shift-and-add (normalised convolution) on device: every clear LR sample of every registered view is placed at
its sub-pixel position on the x2 / x3 / x4 grid, and every HR pixel is the weighted mean of the samples near it - the classical
multi-frame predictor, from exactly what the library already has per batch: `shifts (B,V,2)` of a masked-NCC search, `lr_masks`, `alphas`.

`shift_and_add` is one launch of `hrn_shift_add` behind `torch.ops.hrnet_hip.shift_add`: the views and masks are read once.  The weight
of a sample at distance u (LR pixels, per axis) is k(u) = exp(-u^2 / (2 sigma^2)) cos^2(pi u / 4) inside |u| < 2 (include/hrnet_hip.h
holds the definition); the result is (N + prior base) / (D + prior), D the sum of the weights, so `prior` is the weight of the base frame
in units where one sample at distance 0 weighs 1, and where no sample reaches the result is the base.  It is differentiable in `lrs` and
in a `base` tensor (`hrn_shift_add_backward`, a gather without atomics).  There is NO gradient to shifts, masks or alphas; the forward is
C^1 in the shifts, so that one can follow.  `register_and_add` runs a search against the first view and then the fusion.

The defaults sigma = 0.25 and prior = 0.05 come from a fp64 prototype on ONE SYNTHETIC scene (band-limited, x3, box-averaged views, shifts
within 1.5 px, cloud discs, noise 0.005), where sigma 0.15 .. 0.3 and prior 0 .. 0.2 all beat the bicubic of the clearest view; they are
not tuned on real data.  There is no CPU fallback: tensors must be on a ROCm device."""
import numpy as np
import torch

from . import binding, registration
from .resample import check_scale


def _number(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)):
        raise TypeError(f"{name} must be a number; got {v!r}")
    if not np.isfinite(v):
        raise ValueError(f"{name} must be finite; got {v!r}")
    return float(v)


def check_sigma(sigma):
    sigma = _number("sigma", sigma)
    lo, hi = binding.SHIFT_ADD_SIGMA
    if not lo <= float(np.float32(sigma)) <= hi:
        raise ValueError(f"sigma must lie in [{lo}, {hi}] LR pixels; got {sigma}")
    return sigma


def check_prior(prior):
    prior = _number("prior", prior)
    if prior < 0:
        raise ValueError(f"prior must be >= 0; got {prior}")
    return prior


def shift_and_add(lrs, shifts, lr_masks=None, alphas=None, scale=3, sigma=0.25, prior=0.05, base="bicubic", return_weight=False):
    """lrs (B,V,H,W), shifts (B,V,2) = (dy, dx) as the masked-NCC searches return them (Registered(y,x) = View(y+dy, x+dx)), lr_masks
    (B,V,H,W) 0 / non-zero or None (all clear), alphas (B,V) or None (a view counts iff its alpha is non-zero) -> sr (B, scale H,
    scale W) f32 [, weight (B, scale H, scale W) = the sum of the sample weights at every HR pixel].

    base: "bicubic" - `upsample.baseline(lrs, alphas, lr_masks, scale)`, taken as data; None - no base, and then prior must be 0 (an HR
    pixel no sample reaches is 0); or a (B, scale H, scale W) tensor.  sigma in [0.1, 1] LR pixels, prior >= 0; the defaults are from one
    synthetic scene (see the module's text).  H, W in 1..16384.  Differentiable in lrs and in a base tensor; no gradient to shifts,
    lr_masks or alphas (the forward is C^1 in the shifts).  A view with a non-finite shift contributes nothing."""
    if not torch.is_tensor(lrs):
        raise TypeError(f"lrs must be a torch.Tensor; got {type(lrs).__name__}")
    if lrs.dim() != 4 or lrs.numel() == 0:
        raise ValueError(f"lrs must be a non-empty (B,V,H,W); got {tuple(lrs.shape)}")
    B, V, H, W = lrs.shape
    if not torch.is_tensor(shifts):
        raise TypeError(f"shifts must be a torch.Tensor; got {type(shifts).__name__}")
    if tuple(shifts.shape) != (B, V, 2):
        raise ValueError(f"shifts must be (B,V,2) = {(B, V, 2)}; got {tuple(shifts.shape)}")
    if lr_masks is not None:
        if not torch.is_tensor(lr_masks):
            raise TypeError(f"lr_masks must be a torch.Tensor or None; got {type(lr_masks).__name__}")
        if lr_masks.shape != lrs.shape:
            raise ValueError(f"lr_masks must have the shape of lrs, {tuple(lrs.shape)}; got {tuple(lr_masks.shape)}")
    if alphas is not None:
        if not torch.is_tensor(alphas):
            raise TypeError(f"alphas must be a torch.Tensor or None; got {type(alphas).__name__}")
        if tuple(alphas.shape) != (B, V):
            raise ValueError(f"alphas must be (B,V) = {(B, V)}; got {tuple(alphas.shape)}")
    scale, sigma, prior = check_scale(scale), check_sigma(sigma), check_prior(prior)
    if max(H, W) > binding.SHIFT_ADD_MAX_SIDE:
        raise ValueError(f"frames of 1..{binding.SHIFT_ADD_MAX_SIDE} a side; got {H} x {W}")
    want = (B, scale * H, scale * W)
    if base is None:
        if prior != 0:
            raise ValueError(f"base=None needs prior=0 (there is no frame for the prior to weigh); got prior={prior}")
    elif isinstance(base, str):
        if base != "bicubic":
            raise ValueError(f"base must be \"bicubic\", None or a tensor; got {base!r}")
    elif not torch.is_tensor(base):
        raise TypeError(f"base must be \"bicubic\", None or a torch.Tensor; got {type(base).__name__}")
    elif tuple(base.shape) != want:
        raise ValueError(f"base must be {want} for lrs {tuple(lrs.shape)} at scale {scale}; got {tuple(base.shape)}")
    if not lrs.is_floating_point() or not shifts.is_floating_point() or (torch.is_tensor(base) and not base.is_floating_point()):
        raise TypeError("lrs, shifts and base must be floating-point tensors")
    for name, t in (("lrs", lrs), ("shifts", shifts), ("lr_masks", lr_masks), ("alphas", alphas), ("base", base)):
        if torch.is_tensor(t) and not t.is_cuda:
            raise TypeError(f"{name} is on '{t.device}': shift-and-add runs on a ROCm device only (no CPU fallback)")
        if torch.is_tensor(t) and t.device != lrs.device:
            raise TypeError(f"{name} is on '{t.device}' but lrs on '{lrs.device}'")
    if isinstance(base, str):
        from . import upsample
        with torch.no_grad():
            base = upsample.baseline(lrs, alphas, lr_masks, scale)[:, 0]
    sr, weight = torch.ops.hrnet_hip.shift_add(lrs, lr_masks, alphas, shifts, base, scale, sigma, prior)
    return (sr, weight.detach()) if return_weight else sr            # weight depends on masks and shifts only: no gradient


def register_and_add(lrs, lr_masks=None, alphas=None, scale=3, octaves=0, sigma=0.25, prior=0.05, base="bicubic", **search_kwargs):
    """lrs (B,V,H,W)[, lr_masks, alphas] -> (sr (B, scale H, scale W), weight, shifts (B,V,2)): the views registered against the first
    one (`registration.mncc_search_scene`; with octaves > 0 the coarse-to-fine `mncc_search_pyramid`, whose reach is radius * 2**octaves)
    and fused by `shift_and_add`.  search_kwargs go to the search (points_per_dim, levels, radius, ...); frames are 16..16384 a side,
    the search's limits.  The shifts are found without a gradient; sr is differentiable in lrs at those shifts."""
    registration._no_trace(search_kwargs, "register_and_add returns no trace; call the search itself for it")
    octaves = registration.check_octaves(octaves)
    with torch.no_grad():
        shifts = registration.search_global(lrs, lr_masks, octaves, **search_kwargs)
    sr, weight = shift_and_add(lrs, shifts, lr_masks, alphas, scale, sigma, prior, base, return_weight=True)
    return sr, weight, shifts
