"""Sub-pixel registration of the LR views of an imageset on device: the shift of every view against a reference
frame by a recursive grid search for the maximal masked normalised cross-correlation, and the views resampled by those shifts.

The method is the reference fork's (registration_search.py: compute_shift_ncc -> recursive_mncc_search -> compute_grid_mncc); the
definitions are this project's own and are written out in include/hrnet_hip.h: a six-tap windowed-sinc sampler that is continuous in the
shift and has no padding rule, a bilinear mask sample thresholded at 0.5, and a score standardised on both sides over the common valid
pixels, so that it stays in [-1, 1].  A shift (dy, dx) means Output(y, x) = Input(y + dy, x + dx): the order and sign of
`lanczos_shift`'s argument, the negative of the fork's.

`mncc_search` is one launch of `hrn_mncc_search`: a workgroup owns a view, keeps it in LDS and walks every level, argmax included.
`shift_views` is `hrn_mncc_apply`.  Both are bit-reproducible.  The searches have no autograd formula - a shift found by a grid search
is piecewise constant in the frames - and there is no CPU fallback: tensors must be on a ROCm device.  Frames are 16..128 pixels a side.

The sampler itself is linear in the frame and C^1 in the shift, and `warp` is the resampler with that gradient:
`shift_scene`'s forward, bit for bit, differentiable in the frames and in the shifts (`hrn_mncc_apply_backward`).  It is what a loss on
registered frames, or a shift refined by descent, rests on.  `shift_views`, `shift_scene` and `shift_field` stay without a gradient:
the first two are `warp` without one, and a shift per pixel makes the frames' gradient a scatter, which is not built.

`mncc_search_scene`, `mncc_grid_scene`, `shift_scene` and `register_scene` are the same four for frames of 16..16384 pixels a side
(DESIGN.md section 7g): the scenes `HRNet.forward_tiled` takes, the large benchmark shape, an SR / HR pair.  A frame is cut into tiles
of 64 x 64; a level of the search is two launches and the next level reads its centre from device memory.  Same definitions, same
arguments, same errors; `shift_scene` is bit-identical to `shift_views` where both run.

`mncc_search_local`, `shift_field` and `register_scene_local` find and apply a shift FIELD on the scene path: one
shift per block of `block` x `block` pixels of every view, searched from the view's global shift on the same tiles, and every pixel
resampled by the bilinear field between the blocks' centres.  `local_blocks` is the library's own count of the blocks.

`reduce2`, `mncc_search_pyramid` and `register_scene_pyramid` take the scene search beyond its reach of `radius` <= 4 pixels (DESIGN.md
section 7j): a masked image pyramid of `octaves` 2:1 reductions, the coarsest octave searched from (0, 0) and every finer one from twice
the shift of the octave above - `mncc_search_scene(init=...)`.  The reach is radius * 2**octaves pixels."""
import numpy as np
import torch

from . import binding


def _frames(lrs, lr_masks, scene=False, what="lrs"):
    if not torch.is_tensor(lrs):
        raise TypeError(f"{what} must be a torch.Tensor; got {type(lrs).__name__}")
    if lrs.dim() != 4:
        raise ValueError(f"{what} must be (B,V,H,W); got {tuple(lrs.shape)}")
    if lr_masks is not None:
        if not torch.is_tensor(lr_masks):
            raise TypeError(f"lr_masks must be a torch.Tensor or None; got {type(lr_masks).__name__}")
        if lr_masks.shape != lrs.shape:
            raise ValueError(f"lr_masks must have the shape of {what}, {tuple(lrs.shape)}; got {tuple(lr_masks.shape)}")
    lo, hi = binding.MNCC_SCENE_SIDES if scene else binding.MNCC_SIDES
    if not (lo <= lrs.shape[2] <= hi and lo <= lrs.shape[3] <= hi):
        raise ValueError(f"frames must be {lo}..{hi} pixels a side; got {tuple(lrs.shape[2:])}")


def _reference(lrs, lr_masks, ref, ref_mask):
    """ref=None: the first view and its mask (the loaders order the views from the clearest down)."""
    if ref is None:
        if ref_mask is not None:
            raise ValueError("ref_mask is given without ref: the first view's mask is lr_masks[:, 0]")
        return lrs[:, 0], None if lr_masks is None else lr_masks[:, 0]
    if not torch.is_tensor(ref):
        raise TypeError(f"ref must be a torch.Tensor or None; got {type(ref).__name__}")
    if tuple(ref.shape) != (lrs.shape[0],) + tuple(lrs.shape[2:]):
        raise ValueError(f"ref must be (B,H,W) = {(lrs.shape[0],) + tuple(lrs.shape[2:])}; got {tuple(ref.shape)}")
    if ref_mask is not None:
        if not torch.is_tensor(ref_mask):
            raise TypeError(f"ref_mask must be a torch.Tensor or None; got {type(ref_mask).__name__}")
        if ref_mask.shape != ref.shape:
            raise ValueError(f"ref_mask must have ref's shape {tuple(ref.shape)}; got {tuple(ref_mask.shape)}")
    return ref, ref_mask


def _on_device(**tensors):
    for name, t in tensors.items():
        if t is not None and not t.is_cuda:
            raise TypeError(f"{name} is on '{t.device}': the registration search runs on a ROCm device only (no CPU fallback)")


def _search_args(points_per_dim, levels, radius):
    P = binding.mncc_int("points_per_dim", points_per_dim, binding.MNCC_POINTS)
    levels = binding.mncc_int("levels", levels, binding.MNCC_LEVELS)
    radius = float(radius)
    if not 0.0 < radius <= binding.MNCC_MAX_RADIUS:
        raise ValueError(f"radius must be in (0, {binding.MNCC_MAX_RADIUS:g}]; got {radius}")
    return P, levels, radius


def _problem(scene, lrs, lr_masks, ref, ref_mask, search=()):
    """The opening of every search: the frames, the reference and, where given, `search` = (points_per_dim, levels, radius), checked
    -> (ref, ref_mask) + _search_args(*search).  The caller's own checks come next and _on_device last: a bad argument is reported first."""
    _frames(lrs, lr_masks, scene)
    ref, ref_mask = _reference(lrs, lr_masks, ref, ref_mask)
    return (ref, ref_mask) + (_search_args(*search) if search else ())


def _no_trace(search_kwargs, message):
    if "return_trace" in search_kwargs:
        raise TypeError(message)


def mncc_search(lrs, lr_masks=None, ref=None, ref_mask=None, points_per_dim=7, levels=6, radius=1.0, return_trace=False):
    """lrs (B,V,H,W), lr_masks (B,V,H,W) 0 / non-zero or None (all clear) -> shifts (B,V,2) f32 = (dy, dx): S(view, shift) lies on the
    reference frame.  ref (B,H,W) / ref_mask (B,H,W): the frame to register against; None takes lrs[:, 0] and lr_masks[:, 0].  Level k
    of `levels` searches a points_per_dim^2 grid of width 2 radius s^k around the previous level's best point, s = 1 / (points_per_dim
    - 2) kept within [0.25, 0.9].  return_trace: also (B,V,levels,3) = (dy, dx, score) of every level's best point.  A view without a
    valid score (all zeros, or masked out) gets shift (0, 0) and a score of -inf.  Not differentiable."""
    return _search(False, lrs, lr_masks, ref, ref_mask, points_per_dim, levels, radius, return_trace)


def _init(init, lrs):
    if init is not None:
        if not torch.is_tensor(init):
            raise TypeError(f"init must be a torch.Tensor or None; got {type(init).__name__}")
        if tuple(init.shape) != tuple(lrs.shape[:2]) + (2,):
            raise ValueError(f"init must be (B,V,2) = {tuple(lrs.shape[:2]) + (2,)}; got {tuple(init.shape)}")


def _search(scene, lrs, lr_masks, ref, ref_mask, points_per_dim, levels, radius, return_trace, init=None):
    ref, ref_mask, P, levels, radius = _problem(scene, lrs, lr_masks, ref, ref_mask, (points_per_dim, levels, radius))
    _init(init, lrs)
    _on_device(lrs=lrs, lr_masks=lr_masks, ref=ref, ref_mask=ref_mask, init=init)
    if init is not None:
        shifts, trace = torch.ops.hrnet_hip.mncc_search_scene_from(ref, ref_mask, lrs, lr_masks, init, P, levels, radius)
    else:
        op = torch.ops.hrnet_hip.mncc_search_scene if scene else torch.ops.hrnet_hip.mncc_search
        shifts, trace = op(ref, ref_mask, lrs, lr_masks, P, levels, radius)
    return (shifts, trace) if return_trace else shifts


def mncc_grid(lrs, lr_masks=None, ref=None, ref_mask=None, centres=None, points_per_dim=7, width=2.0):
    """One level of the search, the diagnostic: -> scores (B,V,P,P) f32 at the grid points (cy - width / 2 + i width / (P - 1), cx - width
    / 2 + j width / (P - 1)) around centres (B,V,2) = (cy, cx) (None: zeros); -inf where no pixel is valid or a variance is zero."""
    return _grid(False, lrs, lr_masks, ref, ref_mask, centres, points_per_dim, width)


def _grid(scene, lrs, lr_masks, ref, ref_mask, centres, points_per_dim, width):
    ref, ref_mask = _problem(scene, lrs, lr_masks, ref, ref_mask)
    P = binding.mncc_int("points_per_dim", points_per_dim, binding.MNCC_POINTS)
    width = float(width)
    if not 0.0 < width <= 2.0 * binding.MNCC_MAX_RADIUS:
        raise ValueError(f"width must be in (0, {2.0 * binding.MNCC_MAX_RADIUS:g}]; got {width}")
    if centres is None:
        centres = torch.zeros(tuple(lrs.shape[:2]) + (2,), dtype=torch.float32, device=lrs.device)
    elif not torch.is_tensor(centres):
        raise TypeError(f"centres must be a torch.Tensor or None; got {type(centres).__name__}")
    elif tuple(centres.shape) != tuple(lrs.shape[:2]) + (2,):
        raise ValueError(f"centres must be (B,V,2) = {tuple(lrs.shape[:2]) + (2,)}; got {tuple(centres.shape)}")
    _on_device(lrs=lrs, lr_masks=lr_masks, ref=ref, ref_mask=ref_mask, centres=centres)
    op = torch.ops.hrnet_hip.mncc_grid_scene if scene else torch.ops.hrnet_hip.mncc_grid
    return op(ref, ref_mask, lrs, lr_masks, centres, P, width)


def shift_views(lrs, lr_masks, shifts):
    """-> (registered (B,V,H,W) = S(view, shift), valid (B,V,H,W) f32 0 / 1): the views resampled by shifts (B,V,2) and which of their
    pixels are valid - the six-tap footprint inside the frame and the bilinear sample of the mask above 0.5.  Invalid pixels are 0."""
    return _shift(False, lrs, lr_masks, shifts)


def _shift(scene, lrs, lr_masks, shifts):
    _frames(lrs, lr_masks, scene)
    if not torch.is_tensor(shifts):
        raise TypeError(f"shifts must be a torch.Tensor; got {type(shifts).__name__}")
    if tuple(shifts.shape) != tuple(lrs.shape[:2]) + (2,):
        raise ValueError(f"shifts must be (B,V,2) = {tuple(lrs.shape[:2]) + (2,)}; got {tuple(shifts.shape)}")
    _on_device(lrs=lrs, lr_masks=lr_masks, shifts=shifts)
    return (torch.ops.hrnet_hip.shift_scene if scene else torch.ops.hrnet_hip.shift_views)(lrs, lr_masks, shifts)


def register_views(lrs, lr_masks=None, **search_kwargs):
    """mncc_search, then shift_views by what it found: -> (registered, valid, shifts).  search_kwargs: ref, ref_mask, points_per_dim,
    levels, radius."""
    _no_trace(search_kwargs, "register_views returns no trace: call mncc_search(..., return_trace=True) and shift_views")
    shifts = mncc_search(lrs, lr_masks, **search_kwargs)
    registered, valid = shift_views(lrs, lr_masks, shifts)
    return registered, valid, shifts


# ----------------------------------------------------------------------------- the same four for frames of any size (section 7g)
def mncc_search_scene(lrs, lr_masks=None, ref=None, ref_mask=None, points_per_dim=7, levels=6, radius=1.0, return_trace=False, init=None):
    """`mncc_search` for frames of 16..16384 pixels a side: 1 + 2 levels launches of `hrn_mncc_search_scene` on tiles of 64 x 64, no
    return to the host between them.  The level-k scores are `mncc_grid_scene`'s bit for bit, and a view's result does not depend on
    the batch around it.  init (B,V,2): the first level's centre per view (`hrn_mncc_search_scene_from`); None: (0, 0)."""
    return _search(True, lrs, lr_masks, ref, ref_mask, points_per_dim, levels, radius, return_trace, init)


def mncc_grid_scene(lrs, lr_masks=None, ref=None, ref_mask=None, centres=None, points_per_dim=7, width=2.0):
    """`mncc_grid` for frames of 16..16384 pixels a side.  A grid coordinate beyond +-256 is taken as +-256."""
    return _grid(True, lrs, lr_masks, ref, ref_mask, centres, points_per_dim, width)


def shift_scene(lrs, lr_masks, shifts):
    """`shift_views` for frames of 16..16384 pixels a side; bit-identical to it where both run."""
    return _shift(True, lrs, lr_masks, shifts)


def warp(frames, shifts, masks=None):
    """`shift_scene` as a differentiable function: frames (B,V,H,W) with shifts (B,V,2), or (B,H,W) with shifts (B,2); masks of the
    frames' shape or None -> (warped = S(frame, shift), valid f32 0 / 1), of the frames' shape and with `shift_scene`'s bits.  autograd
    reaches `frames` (the adjoint of the sampler, a gather) and `shifts` (through the derivative of the six taps: the sampler is C^1 in
    the shift, across whole pixels as well) and computes only the half that is needed; `valid` and the masks are piecewise constant
    and carry no gradient.  The gradient that arrives at `warped` counts where `valid` is set, so a loss is the map times `valid`.
    One `hrn_mncc_apply_backward` per backward, bit-reproducible.  A shift of +-256 or beyond has zero slope."""
    if not torch.is_tensor(frames):
        raise TypeError(f"frames must be a torch.Tensor; got {type(frames).__name__}")
    if frames.dim() not in (3, 4):
        raise ValueError(f"frames must be (B,V,H,W) or (B,H,W); got {tuple(frames.shape)}")
    single = frames.dim() == 3
    if single:
        if torch.is_tensor(shifts) and tuple(shifts.shape) != (frames.shape[0], 2):
            raise ValueError(f"shifts must be (B,2) = {(frames.shape[0], 2)}; got {tuple(shifts.shape)}")
        frames = frames[:, None]
        masks = masks[:, None] if torch.is_tensor(masks) and masks.dim() == 3 else masks
        shifts = shifts[:, None] if torch.is_tensor(shifts) else shifts
    _frames(frames, masks, True, "frames")
    if not torch.is_tensor(shifts):
        raise TypeError(f"shifts must be a torch.Tensor; got {type(shifts).__name__}")
    if tuple(shifts.shape) != tuple(frames.shape[:2]) + (2,):
        raise ValueError(f"shifts must be (B,V,2) = {tuple(frames.shape[:2]) + (2,)}; got {tuple(shifts.shape)}")
    _on_device(frames=frames, masks=masks, shifts=shifts)
    warped, valid = torch.ops.hrnet_hip.warp(frames, masks, shifts)
    return (warped[:, 0], valid[:, 0]) if single else (warped, valid)


def register_scene(lrs, lr_masks=None, **search_kwargs):
    """mncc_search_scene, then shift_scene by what it found: -> (registered, valid, shifts).  search_kwargs: ref, ref_mask,
    points_per_dim, levels, radius.  `registered` goes to `HRNet.forward_tiled` as the views did."""
    _no_trace(search_kwargs, "register_scene returns no trace: call mncc_search_scene(..., return_trace=True) and shift_scene")
    shifts = mncc_search_scene(lrs, lr_masks, **search_kwargs)
    registered, valid = shift_scene(lrs, lr_masks, shifts)
    return registered, valid, shifts


# ----------------------------------------------------------------------------- a shift per block of a scene (section 7i)
def local_blocks(H, W, block):
    """-> (by, bx): an axis of length L has max(1, (L + block / 2) // block) blocks of `block` pixels, a multiple of 64 in 64..4096; the
    last block runs to L.  Computed by the library (hrn_mncc_local_blocks)."""
    return binding.mncc_local_blocks(H, W, block)


def _local_args(block, min_valid):
    block, min_valid = binding.mncc_block(block), float(min_valid)
    if not 0.0 <= min_valid <= 1.0:
        raise ValueError(f"min_valid must be in [0, 1]; got {min_valid}")
    return block, min_valid


def mncc_search_local(lrs, lr_masks=None, ref=None, ref_mask=None, block=128, init=None, points_per_dim=7, levels=4, radius=0.5,
                      min_valid=0.25, return_trace=False):
    """-> field (B,V,by,bx,2) f32: per view and block of the frame, the shift of maximal masked NCC with the reference mask restricted to
    the block, by `levels` levels of `mncc_search_scene`'s grid rule around init (B,V,2) - normally the view's global shift; None: zeros.
    A block is ok when its last score is finite and its common valid pixels are at least min_valid of its area; a block that is not ok
    holds init.  The deviation from init is bounded by the sum of the levels' half widths; there is no smoothing.  return_trace: also
    trace (B,V,by,bx,levels,3) = (dy, dx, score) per level and ok (B,V,by,bx) f32 0 / 1.  Not differentiable."""
    ref, ref_mask, P, levels, radius = _problem(True, lrs, lr_masks, ref, ref_mask, (points_per_dim, levels, radius))
    block, min_valid = _local_args(block, min_valid)
    _init(init, lrs)
    _on_device(lrs=lrs, lr_masks=lr_masks, ref=ref, ref_mask=ref_mask, init=init)
    field, trace, ok = torch.ops.hrnet_hip.mncc_search_local(ref, ref_mask, lrs, lr_masks, init, P, levels, radius, block, min_valid)
    return (field, trace, ok) if return_trace else field


def shift_field(lrs, lr_masks, field, block):
    """-> (registered, valid) as `shift_scene`, every pixel by its own shift: field (B,V,by,bx,2) holds the shifts at the centres of the
    blocks' rectangles, bilinear in between and constant beyond the outer centres.  A constant field gives `shift_scene`'s bits."""
    _frames(lrs, lr_masks, True)
    block = binding.mncc_block(block)
    if not torch.is_tensor(field):
        raise TypeError(f"field must be a torch.Tensor; got {type(field).__name__}")
    want = tuple(lrs.shape[:2]) + local_blocks(lrs.shape[2], lrs.shape[3], block) + (2,)
    if tuple(field.shape) != want:
        raise ValueError(f"field must be (B,V,by,bx,2) = {want}; got {tuple(field.shape)}")
    _on_device(lrs=lrs, lr_masks=lr_masks, field=field)
    return torch.ops.hrnet_hip.shift_field(lrs, lr_masks, field, block)


def register_scene_local(lrs, lr_masks=None, block=128, local_levels=4, local_radius=0.5, min_valid=0.25, octaves=0, **search_kwargs):
    """mncc_search_scene with search_kwargs (ref, ref_mask, points_per_dim, levels, radius), mncc_search_local from those shifts with
    local_levels levels of local_radius, then shift_field: -> (registered, valid, field, shifts).  octaves > 0: the global shifts come
    from mncc_search_pyramid over that many octaves instead (search_kwargs then also takes coarse_levels and refine_radius, and radius
    defaults to the pyramid's)."""
    _no_trace(search_kwargs, "register_scene_local returns no trace: call mncc_search_scene and mncc_search_local(..., return_trace=True)")
    _local_args(block, min_valid)
    _search_args(search_kwargs.get("points_per_dim", 7), local_levels, local_radius)
    shifts = search_global(lrs, lr_masks, binding.mncc_int("octaves", octaves, binding.MNCC_OCTAVES), **search_kwargs)
    local = {k: search_kwargs[k] for k in ("ref", "ref_mask", "points_per_dim") if k in search_kwargs}
    field = mncc_search_local(lrs, lr_masks, block=block, init=shifts, levels=local_levels, radius=local_radius, min_valid=min_valid, **local)
    registered, valid = shift_field(lrs, lr_masks, field, block)
    return registered, valid, field, shifts


# ----------------------------------------------------------------------------- coarse to fine: shifts beyond the search's reach (section 7j)
def reduce2(frames, masks=None):
    """frames (B,V,H,W) or (B,H,W), masks of the same shape or None (all clear) -> (reduced, reduced_masks) of (..., H // 2, W // 2): the
    masked [1, 3, 3, 1] / 8 reduction of include/hrnet_hip.h.  A coarse pixel is clear where more than half of its weight lies on clear
    pixels of the frame, and exactly 0 otherwise; the masks come back as f32 1 / 0.  Sides are 32..16384, odd ones allowed.  A shift d
    of the frames is a shift d / 2 of the reduced frames."""
    if not torch.is_tensor(frames):
        raise TypeError(f"frames must be a torch.Tensor; got {type(frames).__name__}")
    if frames.dim() not in (3, 4):
        raise ValueError(f"frames must be (B,V,H,W) or (B,H,W); got {tuple(frames.shape)}")
    if masks is not None:
        if not torch.is_tensor(masks):
            raise TypeError(f"masks must be a torch.Tensor or None; got {type(masks).__name__}")
        if masks.shape != frames.shape:
            raise ValueError(f"masks must have the shape of frames, {tuple(frames.shape)}; got {tuple(masks.shape)}")
    lo, hi = binding.MNCC_REDUCE_SIDES
    H, W = frames.shape[-2:]
    if not (lo <= H <= hi and lo <= W <= hi):
        raise ValueError(f"frames must be {lo}..{hi} pixels a side; got {(H, W)}")
    _on_device(frames=frames, masks=masks)
    out, out_masks = torch.ops.hrnet_hip.reduce2(frames.reshape(-1, H, W), None if masks is None else masks.reshape(-1, H, W))
    shape = tuple(frames.shape[:-2]) + (H // 2, W // 2)
    return out.reshape(shape), out_masks.reshape(shape)


def _pyramid_args(shape, octaves, radius, coarse_levels, refine_radius):
    octaves = binding.mncc_int("octaves", octaves, binding.MNCC_OCTAVES)
    coarse_levels = binding.mncc_int("coarse_levels", coarse_levels, binding.MNCC_LEVELS)
    refine_radius = float(refine_radius)
    if not 0.0 < refine_radius <= binding.MNCC_MAX_RADIUS:
        raise ValueError(f"refine_radius must be in (0, {binding.MNCC_MAX_RADIUS:g}]; got {refine_radius}")
    if radius * 2 ** octaves > binding.MNCC_PYRAMID_MAX_REACH:
        raise ValueError(f"radius * 2**octaves must be at most {binding.MNCC_PYRAMID_MAX_REACH:g} pixels; got {radius} * 2**{octaves}")
    if min(shape[2], shape[3]) >> octaves < binding.MNCC_SCENE_SIDES[0]:
        raise ValueError(f"octave {octaves} of the frames must be at least {binding.MNCC_SCENE_SIDES[0]} pixels a side; the frames are "
                         f"{tuple(shape[2:])}")
    return octaves, coarse_levels, refine_radius


def mncc_search_pyramid(lrs, lr_masks=None, ref=None, ref_mask=None, octaves=2, points_per_dim=7, levels=6, radius=4.0, coarse_levels=3,
                        refine_radius=1.0, return_trace=False):
    """`mncc_search_scene` for shifts of up to radius * 2**octaves pixels (at most 128): -> shifts (B,V,2) f32 in pixels of the frames.
    Octaves 1..octaves of the views and the reference are built with `reduce2`; the coarsest is searched from (0, 0) with `radius`, each
    finer one from twice the shift of the octave above with `refine_radius`; octave 0 takes `levels` levels, the others `coarse_levels`.
    One call of `hrn_mncc_search_pyramid`: nothing returns to the host in between.  octaves=0 is `mncc_search_scene`, bit for bit.
    return_trace: also (B,V,octaves+1,3) = (dy, dx, score) of every octave's last level in that octave's pixels, coarsest first.  Not
    differentiable."""
    ref, ref_mask, P, levels, radius = _problem(True, lrs, lr_masks, ref, ref_mask, (points_per_dim, levels, radius))
    octaves, coarse_levels, refine_radius = _pyramid_args(lrs.shape, octaves, radius, coarse_levels, refine_radius)
    _on_device(lrs=lrs, lr_masks=lr_masks, ref=ref, ref_mask=ref_mask)
    shifts, trace = torch.ops.hrnet_hip.mncc_search_pyramid(ref, ref_mask, lrs, lr_masks, octaves, P, levels, radius, coarse_levels, refine_radius)
    return (shifts, trace) if return_trace else shifts


def check_octaves(octaves):
    """the `octaves` of a function that registers and then fuses (shiftadd.register_and_add, observation.register_and_refine)"""
    if isinstance(octaves, bool) or not isinstance(octaves, (int, np.integer)) or octaves < 0:
        raise ValueError(f"octaves must be an integer >= 0; got {octaves!r}")
    return int(octaves)


def search_global(lrs, lr_masks, octaves, **search_kwargs):
    """-> shifts (B,V,2): the global shift of every view against the first one (or search_kwargs' ref) - `mncc_search_pyramid` over
    `octaves` octaves if octaves > 0, else `mncc_search_scene`.  octaves: an int the caller has checked."""
    if octaves:
        return mncc_search_pyramid(lrs, lr_masks, octaves=octaves, **search_kwargs)
    return mncc_search_scene(lrs, lr_masks, **search_kwargs)


def register_scene_pyramid(lrs, lr_masks=None, **search_kwargs):
    """mncc_search_pyramid, then shift_scene by what it found: -> (registered, valid, shifts).  search_kwargs: ref, ref_mask, octaves,
    points_per_dim, levels, radius, coarse_levels, refine_radius."""
    _no_trace(search_kwargs, "register_scene_pyramid returns no trace: call mncc_search_pyramid(..., return_trace=True) and shift_scene")
    shifts = mncc_search_pyramid(lrs, lr_masks, **search_kwargs)
    registered, valid = shift_scene(lrs, lr_masks, shifts)
    return registered, valid, shifts
