"""The registered-loss tail of a training step on device (reference src/train.py:66-106, :183-187).

`get_loss(srs, hrs, hr_maps, metric, crop)` has the reference's signature (train.py:66) plus `crop`, which folds
`get_crop_mask` (train.py:90-106) into the same pass: callers that multiply the mask themselves pass crop=0.  For 'cMSE' and
'cPSNR' with a gradient-requiring `srs` it is the dispatcher-registered op `torch.ops.hrnet_hip.get_loss_train` (autograd formula: `get_loss_backward`) over `hrn_get_loss_train` / `hrn_get_loss_backward`:
ONE forward pass over the Lanczos output producing n, the brightness bias b and cMSE per sample, and ONE backward pass producing
d(srs) with b held constant - the reference detaches it (train.py:83).  Without gradients (validation) it is the forward-only
`hrn_get_loss`.  No PyTorch fallback.

`shift_loss(srs, hrs, hr_maps, metric, border_w, clip)` is the score the project is judged on, as a loss: shift_cPSNR's search over the
(2 border_w + 1)^2 integer offsets of the target (Evaluator.py:52-73) around the same brightness-corrected cMSE, differentiable through
the selected offset (`torch.ops.hrnet_hip.shift_loss_train` / `.shift_loss_backward`).  It has no parameters, takes frames of any size
and aspect ratio, and is bit-reproducible: the training tail that needs no ShiftNet.

`shift_cssim(srs, hrs, hr_maps, border_w, clip, window, data_range, correct_bias)` is the second score: structural similarity between the
clear pixels of the target and the brightness-corrected prediction, searched over the same offsets (`torch.ops.hrnet_hip.shift_cssim`
over `hrn_shift_cssim`).  It is a score: it has no gradient.

`cssim_loss(srs, hrs, hr_maps, border_w, clip, window, data_range, correct_bias)` is that score as a loss, 1 - cSSIM per sample,
differentiable through the selected offset with the brightness bias attached (`torch.ops.hrnet_hip.shift_cssim_train` /
`.cssim_loss_backward` over `hrn_shift_cssim` / `hrn_cssim_loss_backward`).

`cl1_loss(srs, hrs, hr_maps, border_w, clip, eps)` is the third searched loss: the brightness-corrected L1 (cMAE, eps = 0) or Charbonnier
sqrt(e^2 + eps^2) over the same offsets, the map a weight as in `shift_loss`, to be minimised as it is and differentiable through the
selected offset with the brightness bias attached (`torch.ops.hrnet_hip.cl1_loss_train` / `.cl1_loss_backward` over `hrn_cl1_loss_train`
/ `hrn_cl1_loss_backward`).

`subpixel_loss(srs, hrs, hr_maps, metric, border_w, points_per_dim, levels, radius)` is `shift_loss`'s cMSE / cPSNR with the prediction
registered to its target at a sub-pixel shift: the scene path's grid search scored by the cMSE itself, differentiable through the six-tap
sampler at the point found (`torch.ops.hrnet_hip.subpixel_loss_train` / `.subpixel_loss_backward` over `hrn_subpixel_loss_train` /
`hrn_subpixel_loss_backward`)."""
import torch

from . import binding


def get_loss(srs, hrs, hr_maps, metric="cMSE", crop=0):
    """(B,S,S) x 3 -> (B,) 'masked_MSE' | 'cMSE' | 'cPSNR' (= -10 log10 cMSE, as the reference returns it)."""
    if torch.is_grad_enabled() and torch.is_tensor(srs) and srs.requires_grad:
        if metric == "masked_MSE":
            raise NotImplementedError("masked_MSE has no device backward (train.py only trains on 'cPSNR')")
        out, _stats = torch.ops.hrnet_hip.get_loss_train(srs if srs.dtype == torch.float32 else srs.float(), hrs.float(), hr_maps.float(), metric, int(crop))
        return out
    return binding.get_loss(srs, hrs, hr_maps, metric, crop)


def _searched_inputs(srs, hrs, hr_maps, border_w, noun, window=None):
    """the argument checks of the searched wrappers -> (srs (B,H,W), border_w); `noun`: what the caller computes, for the device error"""
    for name, t in (("srs", srs), ("hrs", hrs), ("hr_maps", hr_maps)):
        if not torch.is_tensor(t):
            raise TypeError(f"{name} must be a torch.Tensor; got {type(t).__name__}")
    if window is not None and window not in binding.CSSIM_WINDOWS:
        raise ValueError(f"window must be one of {sorted(binding.CSSIM_WINDOWS)}; got {window!r}")
    if srs.dim() == 4 and srs.shape[1] == 1:
        srs = srs[:, 0]
    if srs.dim() != 3 or srs.shape != hrs.shape or srs.shape != hr_maps.shape:
        raise ValueError(f"srs, hrs, hr_maps must be equal (B,H,W) tensors; got {tuple(srs.shape)}, {tuple(hrs.shape)}, {tuple(hr_maps.shape)}")
    border_w = int(border_w)
    taps = 1 if window is None else binding.CSSIM_WINDOWS[window][1]
    if border_w < 0 or border_w > 8 or min(srs.shape[1:]) < 2 * border_w + taps:
        if window is None:
            raise ValueError(f"border_w must be 0..8 and smaller than half of each side; got {border_w} for frames {tuple(srs.shape[1:])}")
        raise ValueError(f"border_w must be 0..8 and each side at least 2 border_w + {taps} (the {window} window); got {border_w} for "
                         f"frames {tuple(srs.shape[1:])}")
    for name, t in (("srs", srs), ("hrs", hrs), ("hr_maps", hr_maps)):
        if not t.is_cuda:
            raise TypeError(f"{name} is on '{t.device}': the searched {noun} runs on a ROCm device only (no CPU fallback)")
    return srs, border_w


def _shift_of(stats, border_w):
    """stats' k -> the (B,2) int64 offsets (row, column), as shift_loss returns them"""
    k = stats[:, 3].detach().long()
    nb = 2 * border_w + 1
    return torch.stack([torch.div(k, nb, rounding_mode="floor") - border_w, k % nb - border_w], 1)


def shift_loss(srs, hrs, hr_maps, metric="cPSNR", border_w=3, clip=False, return_shift=False):
    """(B,H,W) x 3 -> (B,): the lowest cMSE over the integer offsets (u - border_w, v - border_w), |.| <= border_w, of `hrs` against the
    centre crop of `srs`, as 'cMSE' or 'cPSNR' (= -10 log10 cMSE, the reference's sign: negate to minimise).  clip clamps srs to [0, 1]
    first, as the scorer does.  A (B,1,H,W) `srs` is taken as srs[:, 0].  With grad enabled and a gradient-requiring `srs` the result
    is differentiable (no gradient to hrs / hr_maps).  return_shift: also the (B,2) int64 offsets (row, column) the loss selected, the
    registration diagnostic ((-border_w - 1, ...) rows mark a sample without a clear pixel, whose loss is NaN)."""
    if metric not in ("cMSE", "cPSNR"):
        raise ValueError(f"metric must be 'cMSE' or 'cPSNR'; got {metric!r}")
    srs, border_w = _searched_inputs(srs, hrs, hr_maps, border_w, "loss")
    srs = srs if srs.dtype == torch.float32 else srs.float()
    if torch.is_grad_enabled() and srs.requires_grad:
        out, stats = torch.ops.hrnet_hip.shift_loss_train(srs.contiguous(), hrs.float().contiguous(), hr_maps.float().contiguous(), metric,
                                                          border_w, bool(clip))
    else:
        out, stats = binding.shift_loss_train(srs, hrs, hr_maps, metric, border_w, clip)
    return (out, _shift_of(stats, border_w)) if return_shift else out


def _cssim_inputs(srs, hrs, hr_maps, border_w, window, data_range):
    """the argument checks of the two cSSIM wrappers -> (srs (B,H,W), border_w, data_range)"""
    data_range = float(data_range)
    if not data_range > 0.0:
        raise ValueError(f"data_range must be positive; got {data_range}")
    srs, border_w = _searched_inputs(srs, hrs, hr_maps, border_w, "score", window)
    return srs, border_w, data_range


def shift_cssim(srs, hrs, hr_maps, border_w=3, clip=True, window="gaussian", data_range=1.0, correct_bias=True, return_shift=False,
                return_scores=False):
    """(B,H,W) x 3 -> (B,): the highest SSIM over the integer offsets (u - border_w, v - border_w), |.| <= border_w, between m hrs and
    m (srs + bias) on the centre crop of `srs`, m the clear pixels of the offset and bias its brightness correction (0 without
    correct_bias).  window: "gaussian" (11 taps, sigma 1.5) or "uniform" (7 taps, sample covariance), over the positions where the
    window fits; data_range: the L of C1 = (0.01 L)^2, C2 = (0.03 L)^2.  clip clamps srs to [0, 1] first.  A (B,1,H,W) `srs` is taken as
    srs[:, 0].  No gradient (`cssim_loss` is the differentiable form).  return_shift: also the (B,2) int64 offsets (row, column)
    selected, as shift_loss returns them (a (-border_w - 1, ...) row marks a sample without an eligible offset, whose score is NaN).
    return_scores: also the (B, (2 border_w + 1)^2) float64 score of every offset, -inf where the offset has no clear pixel."""
    srs, border_w, data_range = _cssim_inputs(srs, hrs, hr_maps, border_w, window, data_range)
    out, stats, scores = torch.ops.hrnet_hip.shift_cssim(srs.detach().float().contiguous(), hrs.float().contiguous(),
                                                         hr_maps.float().contiguous(), border_w, window, bool(clip), bool(correct_bias),
                                                         data_range)
    res = [out]
    if return_shift:
        res.append(_shift_of(stats, border_w))
    if return_scores:
        res.append(scores)
    return res[0] if len(res) == 1 else tuple(res)


def cssim_loss(srs, hrs, hr_maps, border_w=3, clip=False, window="gaussian", data_range=1.0, correct_bias=True, return_shift=False):
    """(B,H,W) x 3 -> (B,): 1 - cSSIM per sample, to be minimised; `shift_cssim`'s arguments, checks and search (clip defaults to False,
    as in shift_loss).  With grad enabled and a gradient-requiring `srs` the result is differentiable through the selected offset, the
    brightness bias attached (`torch.ops.hrnet_hip.shift_cssim_train` / `.cssim_loss_backward`; no gradient to
    hrs / hr_maps); without either it is 1 - shift_cssim(...), the same bits.  The loss is piecewise in the offset, and NaN, with a zero
    gradient, for a sample without an eligible offset.  return_shift: also the (B,2) int64 offsets selected, as in shift_loss."""
    srs, border_w, data_range = _cssim_inputs(srs, hrs, hr_maps, border_w, window, data_range)
    srs = srs if srs.dtype == torch.float32 else srs.float()
    if torch.is_grad_enabled() and srs.requires_grad:
        out, stats = torch.ops.hrnet_hip.shift_cssim_train(srs.contiguous(), hrs.float().contiguous(), hr_maps.float().contiguous(), border_w,
                                                           window, bool(clip), bool(correct_bias), data_range)
    else:
        out, stats, _ = binding.shift_cssim(srs.detach(), hrs, hr_maps, border_w, window, clip, correct_bias, data_range, with_scores=False)
    loss = 1.0 - out
    return (loss, _shift_of(stats, border_w)) if return_shift else loss


def cl1_loss(srs, hrs, hr_maps, border_w=3, clip=False, eps=0.0, return_shift=False):
    """(B,H,W) x 3 -> (B,): the lowest brightness-corrected mean of rho(srs + bias - hrs), weighted by `hr_maps`, over the integer offsets
    (u - border_w, v - border_w), |.| <= border_w, of `hrs` against the centre crop of `srs`; rho(e) = |e| for eps == 0 (cMAE) and
    sqrt(e^2 + eps^2) otherwise (Charbonnier).  To be minimised as it is.  clip clamps srs to [0, 1] first.  A (B,1,H,W) `srs` is taken as
    srs[:, 0].  With grad enabled and a gradient-requiring `srs` the result is differentiable through the selected offset, the bias
    attached (no gradient to hrs / hr_maps); without either the same forward runs and returns the same bits.  NaN,
    with a zero gradient, for a sample without a clear pixel.  return_shift: also the (B,2) int64 offsets selected, as in shift_loss."""
    eps = float(eps)
    if not 0.0 <= eps < float("inf"):
        raise ValueError(f"eps must be finite and not negative; got {eps}")
    srs, border_w = _searched_inputs(srs, hrs, hr_maps, border_w, "loss")
    srs = srs if srs.dtype == torch.float32 else srs.float()
    if torch.is_grad_enabled() and srs.requires_grad:
        out, stats = torch.ops.hrnet_hip.cl1_loss_train(srs.contiguous(), hrs.float().contiguous(), hr_maps.float().contiguous(), border_w,
                                                        bool(clip), eps)
    else:
        out, stats = binding.cl1_loss_train(srs.detach(), hrs, hr_maps, border_w, clip, eps)
    return (out, _shift_of(stats, border_w)) if return_shift else out


def subpixel_loss(srs, hrs, hr_maps, metric="cPSNR", border_w=3, points_per_dim=7, levels=4, radius=3.0, return_shift=False,
                  return_trace=False):
    """(B,H,W) x 3 -> (B,): the brightness-corrected cMSE of the prediction registered to its target at a SUB-PIXEL shift, as 'cMSE' or
    'cPSNR' (= -10 log10 cMSE, the reference's sign: negate to minimise).  The shift s* = (dy, dx) is found on device by `levels` grids of
    points_per_dim^2 points, the first of width 2 radius around (0, 0), each around the best point of the one before - the search of
    `registration.mncc_search_scene`, scored by the cMSE of S(srs, s) against `hrs` over the clear pixels (hr_maps != 0, binary) at
    least border_w from every edge whose six-tap footprint lies inside the frame.  Frames of 16..16384 pixels a
    side, border_w 0..8 and below half of each side, points_per_dim 3..9, levels 1..16, radius in (0, 4]; there is no `clip`.  A
    (B,1,H,W) `srs` is taken as srs[:, 0].  With grad enabled and a gradient-requiring `srs` the result is differentiable through the
    sampler at s*, which is held fixed (no gradient to hrs / hr_maps or to the shift); without either the same forward runs and returns
    the same bits - the sub-pixel score diagnostic.  NaN, with a zero gradient, for a sample without a counted pixel.
    return_shift: also the (B,2) float32 s*.  S(srs, s)(p) = srs(p + s), so s* is the NEGATIVE of the (row, column) offset `shift_loss`
    selects, which pairs srs(p) with hrs(p + offset): for a whole-pixel misregistration within both reaches, round(s*) = -offset.
    return_trace: also the (B,levels,3) float32 (dy, dx, cMSE) of every level's point."""
    if metric not in ("cMSE", "cPSNR"):
        raise ValueError(f"metric must be 'cMSE' or 'cPSNR'; got {metric!r}")
    P = binding.mncc_int("points_per_dim", points_per_dim, binding.MNCC_POINTS)
    levels, radius = binding.mncc_int("levels", levels, binding.MNCC_LEVELS), float(radius)
    if not 0.0 < radius <= binding.MNCC_MAX_RADIUS:
        raise ValueError(f"radius must be in (0, {binding.MNCC_MAX_RADIUS:g}]; got {radius}")
    lo, hi = binding.MNCC_SCENE_SIDES
    if torch.is_tensor(srs) and srs.dim() >= 2 and not (lo <= min(srs.shape[-2:]) and max(srs.shape[-2:]) <= hi):
        raise ValueError(f"the sides of a frame must be {lo}..{hi}; got {tuple(srs.shape[-2:])}")
    srs, border_w = _searched_inputs(srs, hrs, hr_maps, border_w, "loss")
    srs = srs if srs.dtype == torch.float32 else srs.float()
    if torch.is_grad_enabled() and srs.requires_grad:
        out, stats, trace = torch.ops.hrnet_hip.subpixel_loss_train(srs.contiguous(), hrs.float().contiguous(), hr_maps.float().contiguous(),
                                                                    metric, border_w, P, levels, radius)
    else:
        out, stats, trace = binding.subpixel_loss_train(srs.detach(), hrs, hr_maps, metric, border_w, P, levels, radius)
    res = [out]
    if return_shift:
        res.append(stats[:, 3:5].detach().float())
    if return_trace:
        res.append(trace.detach())
    return res[0] if len(res) == 1 else tuple(res)
