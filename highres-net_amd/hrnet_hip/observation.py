"""The observation model on device: what every registered LR view should have recorded of an HR frame, the
data-consistency loss that compares it with the views themselves, and iterative back-projection - the way back from the HR grid that
shift-and-add (`shiftadd`) lacks.

`A_v x`: view sample i integrates the HR frame over one LR pixel, as `scale` point samples per axis at the HR coordinates
`scale (i - dy) + k`, each read with the six-tap sampler of the registration code and averaged - a separable (scale + 5)-tap filter per
view and a decimation (include/hrnet_hip.h holds the definition).  `shifts (B,V,2)` are what any masked-NCC search returns
(Registered(y,x) = View(y+dy, x+dx)); there is no padding rule, so a sample whose footprint leaves the HR frame is not valid.

`observe` makes synthetic LR views of HR frames; `consistency_loss` is `sum_v |counted (A_v sr - lr_v + beta_v)|^2 / sum_v n_v`, a loss
without an HR target (self-supervised fine-tuning, PROBA-V's test split) with the brightness bias beta_v every loss here corrects;
`back_project` refines a frame against the views, `x <- x - step (scale^2 / V_b) sum_v A_v^T r_v`; `register_and_refine` registers,
starts from shift-and-add or the bicubic baseline and refines.  Gradients go to the HR frame and - with shift_grad=True, DESIGN.md section
7v - to the shifts; there is NONE to lrs, masks or alphas.  `shift_normal`, `refine_shifts` and `reconstruct_joint` use the same derivative
for Gauss-Newton steps on the shifts: joint estimation of the frame and its registration.  There is no CPU fallback: tensors must be on a
ROCm device."""
import numpy as np
import torch

from . import binding, registration
from .resample import check_scale


def _tensor(name, t, shape=None, optional=False):
    if t is None and optional:
        return
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a torch.Tensor{' or None' if optional else ''}; got {type(t).__name__}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be {tuple(shape)}; got {tuple(t.shape)}")


def _on_device(first, **tensors):
    for name, t in tensors.items():
        if not torch.is_tensor(t):
            continue
        if not t.is_cuda:
            raise TypeError(f"{name} is on '{t.device}': the observation model runs on a ROCm device only (no CPU fallback)")
        if t.device != first.device:
            raise TypeError(f"{name} is on '{t.device}' but the first argument on '{first.device}'")


def _flag(name, v):
    if not isinstance(v, (bool, np.bool_)):
        raise TypeError(f"{name} must be a bool; got {v!r}")
    return bool(v)


def check_step(step):
    if isinstance(step, bool) or not isinstance(step, (int, float, np.floating, np.integer)):
        raise TypeError(f"step must be a number; got {step!r}")
    lo, hi = binding.OBSERVE_STEP
    if not (np.isfinite(step) and lo < float(np.float32(step)) < hi):
        raise ValueError(f"step must lie in ({lo}, {hi}); got {step}")
    return float(step)


def check_iters(iters):
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or iters < 0:
        raise ValueError(f"iters must be an integer >= 0; got {iters!r}")
    return int(iters)


def _check_views(srs, lrs, shifts, lr_masks, alphas, scale, what="srs"):
    """the checks every function with LR views shares -> (srs as (B,SH,SW), whether it came as (B,1,SH,SW), scale)"""
    _tensor(what, srs)
    _tensor("lrs", lrs)
    if lrs.dim() != 4 or lrs.numel() == 0:
        raise ValueError(f"lrs must be a non-empty (B,V,H,W); got {tuple(lrs.shape)}")
    B, V, H, W = lrs.shape
    scale = check_scale(scale)
    channel = srs.dim() == 4
    if channel and srs.shape[1] != 1:
        raise ValueError(f"{what} must be (B,SH,SW) or (B,1,SH,SW); got {tuple(srs.shape)}")
    want = (B, scale * H, scale * W)
    if tuple(srs.shape) not in (want, (B, 1) + want[1:]):
        raise ValueError(f"{what} must be {want} (or with a channel of 1) for lrs {tuple(lrs.shape)} at scale {scale}; got {tuple(srs.shape)}")
    _tensor("shifts", shifts, (B, V, 2))
    _tensor("lr_masks", lr_masks, lrs.shape, optional=True)
    _tensor("alphas", alphas, (B, V), optional=True)
    if max(H, W) > binding.OBSERVE_MAX_SIDE:
        raise ValueError(f"frames of 1..{binding.OBSERVE_MAX_SIDE} a side; got {H} x {W}")
    if not (srs.is_floating_point() and lrs.is_floating_point() and shifts.is_floating_point()):
        raise TypeError(f"{what}, lrs and shifts must be floating-point tensors")
    _on_device(srs, lrs=lrs, shifts=shifts, lr_masks=lr_masks, alphas=alphas, **{what: srs})
    return (srs[:, 0] if channel else srs), channel, scale


def observe(hr, shifts, scale=3, shift_grad=False):
    """hr (B, scale H, scale W), shifts (B,V,2) -> (views (B,V,H,W), valid (B,V,H,W) f32 0 / 1): what a view at each shift records of the
    HR frame - synthetic LR views with the library's own sampler.  A sample whose footprint leaves the frame is 0 and not valid, and so is
    every sample of a view with a non-finite shift (or one of 256 / scale LR pixels or more).  Differentiable in hr (the adjoint kernel);
    the gradient that arrives at `views` counts where `valid` is set.  shift_grad: the same bits, differentiable in shifts too (the
    operator is C^1 in them; `valid` is piecewise constant and not differentiated), each gradient computed only when it is needed.  The HR
    sides must be multiples of scale, H, W in 1..16384."""
    shift_grad = _flag("shift_grad", shift_grad)
    _tensor("hr", hr)
    _tensor("shifts", shifts)
    scale = check_scale(scale)
    if hr.dim() != 3 or hr.numel() == 0:
        raise ValueError(f"hr must be a non-empty (B,SH,SW); got {tuple(hr.shape)}")
    if hr.shape[1] % scale or hr.shape[2] % scale:
        raise ValueError(f"the sides of hr must be multiples of scale {scale}; got {tuple(hr.shape)}")
    if shifts.dim() != 3 or shifts.shape[0] != hr.shape[0] or shifts.shape[1] == 0 or shifts.shape[2] != 2:
        raise ValueError(f"shifts must be (B,V,2) with B = {hr.shape[0]} and V >= 1; got {tuple(shifts.shape)}")
    if max(hr.shape[1:]) > scale * binding.OBSERVE_MAX_SIDE:
        raise ValueError(f"LR frames of 1..{binding.OBSERVE_MAX_SIDE} a side; got hr {tuple(hr.shape)} at scale {scale}")
    if not (hr.is_floating_point() and shifts.is_floating_point()):
        raise TypeError("hr and shifts must be floating-point tensors")
    _on_device(hr, hr=hr, shifts=shifts)
    if shift_grad:
        views, valid = torch.ops.hrnet_hip.observe_sg(hr, shifts, scale)
    else:
        views, valid = torch.ops.hrnet_hip.observe(hr, shifts.detach(), scale)
    return views, valid.detach()


def consistency_loss(srs, lrs, shifts, lr_masks=None, alphas=None, scale=3, brightness=True, return_residual=False, shift_grad=False):
    """srs (B,SH,SW) or (B,1,SH,SW), lrs (B,V,H,W), shifts (B,V,2)[, lr_masks (B,V,H,W) 0 / non-zero, alphas (B,V): a view counts iff its
    alpha is non-zero] -> loss (B,) = sum_v sum (counted (A_v sr - lr_v + beta_v))^2 / sum_v n_v, exactly 0 for a sample in which nothing
    counts.  brightness: beta_v = -mean of the counted A_v sr - lr_v (the views' brightness bias), else 0.  return_residual: also
    (residual (B,V,H,W) = A_v sr - lr_v where counted and 0 elsewhere, beta (B,V), count (B,V) int32), all without a gradient.
    Differentiable in srs only; with shift_grad the same bits, differentiable in shifts too (the loss a registration network can be
    trained on without an HR target).  Two launches forward (nothing returns to the host), one backward, two more for d_shifts."""
    brightness, shift_grad = _flag("brightness", brightness), _flag("shift_grad", shift_grad)
    srs3, _, scale = _check_views(srs, lrs, shifts, lr_masks, alphas, scale)
    det = lambda t: None if t is None else t.detach()
    if shift_grad:
        op, sh = torch.ops.hrnet_hip.consistency_loss_sg, shifts
    else:
        op, sh = torch.ops.hrnet_hip.consistency_loss_train, shifts.detach()
    loss, residual, beta, count, _ = op(srs3, lrs.detach(), det(lr_masks), det(alphas), sh, scale, brightness)
    return (loss, residual.detach(), beta.detach(), count) if return_residual else loss


def back_project(sr0, lrs, shifts, lr_masks=None, alphas=None, scale=3, iters=10, step=1.0, brightness=True, return_loss=False):
    """sr0 (B,SH,SW) or (B,1,SH,SW) -> sr of the same shape after `iters` steps x <- x - step (scale^2 / V_b) sum_v A_v^T r_v(x), V_b the
    number of views with a counted pixel (a sample without one is returned unchanged).  step in (0, 2): the largest eigenvalue of
    (scale^2 / V) sum_v A_v^T M A_v is 1 within 2 %.  iters = 0 returns sr0's bits.  return_loss: also losses (iters,B), the
    consistency loss of the frame every step started from, on the device.  No gradient.  3 iters launches on the current stream."""
    iters, step, brightness = check_iters(iters), check_step(step), _flag("brightness", brightness)
    srs3, channel, scale = _check_views(sr0, lrs, shifts, lr_masks, alphas, scale, what="sr0")
    with torch.no_grad():
        sr, losses = torch.ops.hrnet_hip.back_project(srs3, lrs, lr_masks, alphas, shifts, scale, iters, step, brightness)
    sr = sr.unsqueeze(1) if channel else sr
    return (sr, losses) if return_loss else sr


def _number(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)):
        raise TypeError(f"{name} must be a number; got {v!r}")
    if not np.isfinite(v):
        raise ValueError(f"{name} must be finite; got {v}")
    return float(v)


def check_btv(P, alpha, eps):
    """the bilateral-TV window: P in 1..3, 0 < alpha <= 1, eps > 0 -> (P, alpha, eps)"""
    if isinstance(P, bool) or not isinstance(P, (int, np.integer)) or not 1 <= P <= binding.BTV_MAX_P:
        raise ValueError(f"P must be an integer in 1..{binding.BTV_MAX_P}; got {P!r}")
    alpha, eps = _number("alpha", alpha), _number("eps", eps)
    if not 0.0 < alpha <= 1.0:
        raise ValueError(f"alpha must lie in (0, 1]; got {alpha}")
    if not eps > 0.0:
        raise ValueError(f"eps must be positive; got {eps}")
    return int(P), alpha, eps


def check_reconstruct(step, robust, delta, lam, P, alpha, eps):
    """the options of `reconstruct` -> (step, robust as a bool, delta, lam, P, alpha, eps).  The step-size rule: the Hessian of lam R is
    bounded by 4 lam W / eps, W = sum_{(l,m) != 0} alpha^(|l|+|m|), the data operator's largest eigenvalue by 1.02, so
    step (1.02 + 4 lam W / eps) must stay below 2."""
    step = check_step(step)
    if robust not in (None, "welsch"):
        raise ValueError(f"robust must be None or \"welsch\"; got {robust!r}")
    delta, lam = _number("delta", delta), _number("lam", lam)
    if not delta > 0.0:
        raise ValueError(f"delta must be positive; got {delta}")
    if lam < 0.0:
        raise ValueError(f"lam must be >= 0; got {lam}")
    P, alpha, eps = check_btv(P, alpha, eps)
    if lam > 0.0:
        W = binding.btv_weight_sum(P, alpha)
        bound = binding.step_bound(step, lam, P, alpha, eps)
        if not bound < 2.0:
            raise ValueError(f"step (1.02 + 4 lam W / eps) must be below 2 for the iteration to be stable; got {bound:.4g} from step={step}, "
                             f"lam={lam}, W={W:.4g} (P={P}, alpha={alpha}), eps={eps}: lower step or lam, or raise eps")
    return step, robust is not None, delta, lam, P, alpha, eps


def reconstruct(sr0, lrs, shifts, lr_masks=None, alphas=None, scale=3, iters=30, step=1.0, brightness=True, robust="welsch", delta=0.1,
                lam=4e-4, P=2, alpha=0.7, eps=0.02, return_trace=False):
    """sr0 (B,SH,SW) or (B,1,SH,SW) -> sr of the same shape after `iters` iterations of a robust, regularised back-projection.
    Each iteration takes a data step and, with lam > 0, a bilateral-TV half-step evaluated at the data step's result (a splitting scheme):
      data step, robust="welsch": w = counted exp(-((e + beta_prev) / delta)^2), beta_v = -sum w e / sum w (0 without `brightness`),
        x' = x - step (scale^2 / V_b) sum_v A_v^T (w (e + beta_v)); beta_prev starts as the plain mean bias of the first iteration.  A
        redescending weight: a pixel far from the model (an unmasked cloud) loses its pull, and the bias is not contaminated by it.
        robust=None: back_project's step.  A sample in which nothing counts takes no data step.
      prior: x'' = x' - step lam g(x'), g the gradient of R(x) = sum_{(l,m) != 0, |l|,|m| <= P} alpha^(|l|+|m|) sum_p phi(x_p - x_{p-(l,m)}),
        phi(t) = sqrt(t^2 + eps^2) - eps, pairs inside the frame only.  A sample in which nothing counts STILL takes this half-step.
    step (1.02 + 4 lam W / eps) must stay below 2 (ValueError otherwise; W = sum of the window's weights, 10.42 for P=2, alpha=0.7).
    robust=None, lam=0 returns back_project's bits; iters = 0 returns sr0's bits.  return_trace: also trace (iters,B,3) on the device =
    (the plain consistency loss, the weighted loss sum w (e + beta_prev)^2 / sum w, lam R / pixels) of the frame each iteration started
    from.  No gradient.  Per iteration 3 launches, 6 with robust, 1 more with lam > 0 (2 more with return_trace), on the current stream."""
    iters, brightness = check_iters(iters), _flag("brightness", brightness)
    return_trace = _flag("return_trace", return_trace)
    step, robust, delta, lam, P, alpha, eps = check_reconstruct(step, robust, delta, lam, P, alpha, eps)
    srs3, channel, scale = _check_views(sr0, lrs, shifts, lr_masks, alphas, scale, what="sr0")
    with torch.no_grad():
        sr, trace = torch.ops.hrnet_hip.reconstruct(srs3, lrs, lr_masks, alphas, shifts, scale, iters, step, brightness, robust, delta, lam, P,
                                                    alpha, eps, return_trace)
    sr = sr.unsqueeze(1) if channel else sr
    return (sr, trace) if return_trace else sr


def check_refine(damping, max_step, delta, robust):
    """the options of the shift update -> (damping, max_step, delta, robust as a bool): damping >= 0, max_step > 0 (LR pixels), delta > 0"""
    damping, max_step, delta = _number("damping", damping), _number("max_step", max_step), _number("delta", delta)
    if damping < 0.0:
        raise ValueError(f"damping must be >= 0; got {damping}")
    if not max_step > 0.0:
        raise ValueError(f"max_step must be positive; got {max_step}")
    if not delta > 0.0:
        raise ValueError(f"delta must be positive; got {delta}")
    if robust not in (None, "welsch"):
        raise ValueError(f"robust must be None or \"welsch\"; got {robust!r}")
    return damping, max_step, delta, robust is not None


def _check_fixed(fixed, lrs):
    """`fixed` is a view index, None, or a (B,V) bool tensor (judged before any device is asked for)"""
    if fixed is None or not torch.is_tensor(lrs) or lrs.dim() != 4:
        return
    B, V = lrs.shape[:2]
    if torch.is_tensor(fixed):
        if tuple(fixed.shape) != (B, V) or fixed.dtype != torch.bool:
            raise ValueError(f"fixed must be a view index, None or a ({B}, {V}) bool tensor; got {tuple(fixed.shape)} {fixed.dtype}")
    elif isinstance(fixed, bool) or not isinstance(fixed, (int, np.integer)) or not 0 <= fixed < V:
        raise ValueError(f"fixed must be a view index in 0..{V - 1}, None or a ({B}, {V}) bool tensor; got {fixed!r}")


def _fixed_views(fixed, B, V, first):
    """a checked `fixed` -> (B,V) uint8 on the device of `first`, or None"""
    if fixed is None:
        return None
    if torch.is_tensor(fixed):
        _on_device(first, fixed=fixed)
        return fixed.to(torch.uint8).contiguous()
    mask = torch.zeros((B, V), dtype=torch.uint8, device=first.device)
    mask[:, int(fixed)] = 1
    return mask


def shift_normal(sr, lrs, shifts, lr_masks=None, alphas=None, scale=3, brightness=True, robust=None, delta=0.1, beta_prev=None):
    """-> normal (B,V,8) fp64 = [sum p, g_y, g_x, H_yy, H_yx, H_xx, beta, sum p (e + beta)^2], the normal equations of every view's shift
    against the frame sr (a diagnostic): p = counted, or with robust="welsch" the Welsch weight of e + beta_prev (beta_prev
    (B,V); None: the plain mean bias of this frame, what `reconstruct`'s first iteration uses).  With `brightness` the bias is projected
    out of the derivative images.  No gradient.  Two launches (four with robust and no beta_prev)."""
    brightness = _flag("brightness", brightness)
    _, _, delta, robust = check_refine(0.0, 1.0, delta, robust)
    if beta_prev is not None and not robust:
        raise ValueError("beta_prev is the state of robust=\"welsch\"; got robust=None")
    srs3, _, scale = _check_views(sr, lrs, shifts, lr_masks, alphas, scale, what="sr")
    _tensor("beta_prev", beta_prev, shifts.shape[:2], optional=True)
    _on_device(sr, beta_prev=beta_prev)
    with torch.no_grad():
        if robust and beta_prev is None:
            beta_prev = torch.ops.hrnet_hip.consistency_loss_train(srs3, lrs, lr_masks, alphas, shifts, scale, brightness)[2]
        return torch.ops.hrnet_hip.shift_normal(srs3, lrs, lr_masks, alphas, shifts, beta_prev, scale, brightness, delta)


def refine_shifts(sr, lrs, shifts, lr_masks=None, alphas=None, scale=3, iters=2, damping=1e-3, max_step=0.5, fixed=0, brightness=True,
                  robust=None, delta=0.1, return_trace=False):
    """-> shifts' (B,V,2) after `iters` Levenberg-damped Gauss-Newton steps on every view's shift against the frame sr, which is held
    (DESIGN 7v): step = -(H + damping tr(H) / 2 I)^-1 g, its largest component at most max_step LR pixels.  fixed: a view index, None, or a
    (B,V) bool tensor - view 0 by default, the gauge: a common translation of all views and the frame is otherwise free.  A view keeps
    its shift's bits when it is fixed, does not count, has fewer than 3 pixels' weight, or its damped system is singular.  It repairs
    rough shifts (about 0.3 px off); it does NOT improve on a good masked-NCC search.  return_trace: also (iters,B,V,8) fp64, the normal
    equations every step started from.  No gradient; nothing returns to the host.  Two launches a step (four with robust)."""
    iters, brightness, return_trace = check_iters(iters), _flag("brightness", brightness), _flag("return_trace", return_trace)
    damping, max_step, delta, robust = check_refine(damping, max_step, delta, robust)
    _check_fixed(fixed, lrs)
    srs3, _, scale = _check_views(sr, lrs, shifts, lr_masks, alphas, scale, what="sr")
    fixed = _fixed_views(fixed, lrs.shape[0], lrs.shape[1], sr)
    with torch.no_grad():
        out, trace = torch.ops.hrnet_hip.refine_shifts(srs3, lrs, lr_masks, alphas, shifts, fixed, scale, iters, damping, max_step, brightness,
                                                       robust, delta)
    return (out, trace) if return_trace else out


def reconstruct_joint(sr0, lrs, shifts, lr_masks=None, alphas=None, scale=3, iters=30, refine_every=1, refine_from=1, damping=1e-3,
                      max_step=0.5, fixed=0, step=1.0, brightness=True, robust="welsch", delta=0.1, lam=4e-4, P=2, alpha=0.7, eps=0.02):
    """-> (sr, shifts): `reconstruct`'s iteration with a Gauss-Newton update of the shifts (`refine_shifts`' step) beside the data step of
    iteration t = refine_from, refine_from + refine_every, ... (0-based); both read the frame and the shifts the iteration started from.
    In Welsch mode the update's weights need a beta_prev, so iteration 0 never updates.  refine_every = 0 returns `reconstruct`'s bits and
    the input shifts' bits.  The other options are `reconstruct`'s and `refine_shifts`'.  No gradient.  Per iteration `reconstruct`'s
    launches; an iteration that updates runs the normal pass in place of the residual pass (one pass over the frame) and one launch more."""
    iters, brightness = check_iters(iters), _flag("brightness", brightness)
    for name, v in (("refine_every", refine_every), ("refine_from", refine_from)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
            raise ValueError(f"{name} must be an integer >= 0; got {v!r}")
    refine_every, refine_from = int(refine_every), int(refine_from)
    damping, max_step, _, _ = check_refine(damping, max_step, delta, robust)
    step, robust, delta, lam, P, alpha, eps = check_reconstruct(step, robust, delta, lam, P, alpha, eps)
    _check_fixed(fixed, lrs)
    srs3, channel, scale = _check_views(sr0, lrs, shifts, lr_masks, alphas, scale, what="sr0")
    fixed = _fixed_views(fixed, lrs.shape[0], lrs.shape[1], sr0)
    with torch.no_grad():
        sr, out = torch.ops.hrnet_hip.reconstruct_joint(srs3, lrs, lr_masks, alphas, shifts, fixed, scale, iters, refine_every, refine_from,
                                                        damping, max_step, step, brightness, robust, delta, lam, P, alpha, eps)
    return (sr.unsqueeze(1) if channel else sr), out


def btv_loss(srs, P=2, alpha=0.7, eps=0.02):
    """srs (B,SH,SW) or (B,1,SH,SW) -> (B,) = R(srs_b) / (SH SW), the bilateral-TV prior of `reconstruct` as a training regulariser beside
    any loss here.  Differentiable in srs (the half-step's kernel with out = gain g).  Sides of 1..49152."""
    _tensor("srs", srs)
    P, alpha, eps = check_btv(P, alpha, eps)
    if srs.dim() == 4 and srs.shape[1] == 1:
        srs = srs[:, 0]
    if srs.dim() != 3 or srs.numel() == 0:
        raise ValueError(f"srs must be a non-empty (B,SH,SW) or (B,1,SH,SW); got {tuple(srs.shape)}")
    if max(srs.shape[1:]) > binding.BTV_MAX_SIDE:
        raise ValueError(f"planes of 1..{binding.BTV_MAX_SIDE} a side; got {tuple(srs.shape)}")
    if not srs.is_floating_point():
        raise TypeError("srs must be a floating-point tensor")
    _on_device(srs, srs=srs)
    return torch.ops.hrnet_hip.btv_loss_train(srs, P, alpha, eps)


def register_and_refine(lrs, lr_masks=None, alphas=None, scale=3, iters=10, step=1.0, init="shift_add", octaves=0, robust=None, delta=0.1,
                        lam=0.0, P=2, alpha=0.7, eps=0.02, joint=False, **search_kwargs):
    """lrs (B,V,H,W)[, lr_masks, alphas] -> (sr (B, scale H, scale W), shifts (B,V,2)): the views registered against the first one, a
    start - init="shift_add": `shiftadd.register_and_add`; "bicubic": the search (`registration.mncc_search_scene`, or with octaves > 0
    `mncc_search_pyramid`) and `upsample.baseline` - and `iters` back-projection steps from it; with robust="welsch" or lam > 0 the
    iterations are `reconstruct`'s (delta, lam, P, alpha, eps are its).  search_kwargs go to the search; frames are 16..16384 a side, the
    search's limits.  joint: the iterations are `reconstruct_joint`'s with its defaults (view 0 fixed), and the shifts returned are the
    refined ones - for rough shifts; it does not improve on a search that worked.  No gradient."""
    joint = _flag("joint", joint)
    if init not in ("shift_add", "bicubic"):
        raise ValueError(f"init must be \"shift_add\" or \"bicubic\"; got {init!r}")
    iters, step, scale = check_iters(iters), check_step(step), check_scale(scale)
    check_reconstruct(step, robust, delta, lam, P, alpha, eps)
    registration._no_trace(search_kwargs, "register_and_refine returns no trace; call the search itself for it")
    octaves = registration.check_octaves(octaves)
    from . import shiftadd, upsample
    with torch.no_grad():
        if init == "shift_add":
            sr0, _, shifts = shiftadd.register_and_add(lrs, lr_masks, alphas, scale=scale, octaves=octaves, **search_kwargs)
        else:
            shifts = registration.search_global(lrs, lr_masks, octaves, **search_kwargs)
            sr0 = upsample.baseline(lrs, alphas, lr_masks, scale)[:, 0]
        if joint:
            sr, shifts = reconstruct_joint(sr0, lrs, shifts, lr_masks, alphas, scale, iters, step=step, robust=robust, delta=delta, lam=lam, P=P,
                                           alpha=alpha, eps=eps)
        elif robust is None and lam == 0:
            sr = back_project(sr0, lrs, shifts, lr_masks, alphas, scale, iters, step)
        else:
            sr = reconstruct(sr0, lrs, shifts, lr_masks, alphas, scale, iters, step, True, robust, delta, lam, P, alpha, eps)
    return sr, shifts
