"""The coarse-to-fine masked-NCC search restated in numpy fp64 (the definitions are in include/hrnet_hip.h), for the
tests of hrnet_hip.registration's reduce2 / mncc_search_scene(init=...) / mncc_search_pyramid: the masked [1, 3, 3, 1] / 8 reduction, the
search of registration_ref from a given centre, the pyramid over both, and scenes whose views lie tens of pixels apart.  Built on
registration_ref's grid, best_of and level_widths.  No test logic here."""
import numpy as np

import registration_ref as R

WEIGHTS = np.array([1.0, 3.0, 3.0, 1.0]) / 8.0
# reduce2 against fp64 on values in [0, 1): 1.67e-7 is the largest |device - fp64| measured on an MI355X over the five shapes, four
# alignments and both mask forms of tests/test_gpu_registration_pyramid.py (under three ulp of a value in 0.5..1: sixteen fused
# multiply-adds and one divide); times 4, rounded up to one digit, and under the cap of 1e-6.  The neighbour of tests/kernel_bounds.py's
# figures.
REDUCE2_BOUND = 7e-7


def reduce2(x, mask=None):
    """(H, W) with a mask (0 / non-zero, None: all clear) -> (value (H // 2, W // 2) float64, clear (H // 2, W // 2) bool, den float64).
    Coarse pixel (Y, X) reads fine rows 2Y - 1 .. 2Y + 2 and columns 2X - 1 .. 2X + 2 with weights w_a w_b; m = inside the frame and
    clear; den = sum w m, num = sum w (m ? x : 0); clear iff den > 0.5; value = num / den where clear and 0 elsewhere."""
    x = np.asarray(x, np.float64)
    H, W = x.shape
    Ho, Wo = H // 2, W // 2
    m = np.ones((H, W), bool) if mask is None else np.asarray(mask) != 0
    pm, px = np.zeros((H + 3, W + 3)), np.zeros((H + 3, W + 3))          # the frame at (1, 1): one pixel before, two after
    pm[1:H + 1, 1:W + 1] = m
    px[1:H + 1, 1:W + 1] = np.where(m, x, 0.0)
    den, num = np.zeros((Ho, Wo)), np.zeros((Ho, Wo))
    for a in range(4):
        for b in range(4):
            w = WEIGHTS[a] * WEIGHTS[b]
            den += w * pm[a:a + 2 * Ho:2, b:b + 2 * Wo:2]
            num += w * px[a:a + 2 * Ho:2, b:b + 2 * Wo:2]
    clear = den > 0.5
    return np.where(clear, num / np.where(clear, den, 1.0), 0.0), clear, den


def search_from(ref, ref_mask, view, view_mask, init, P=7, levels=6, radius=1.0):
    """registration_ref.search with the first centre `init` = (cy, cx) instead of (0, 0): -> (shift (2,) fp32, trace (levels, 3))."""
    centre = (np.float32(init[0]), np.float32(init[1]))
    trace = np.zeros((levels, 3))
    for k, w in enumerate(R.level_widths(P, levels, radius)):
        s, dys, dxs = R.grid(ref, ref_mask, view, view_mask, centre, w, P)
        centre, best = R.best_of(s, dys, dxs, centre)
        trace[k] = (centre[0], centre[1], best)
    return np.array(centre, np.float32), trace


def octaves_of(x, mask, K):
    """[(x, mask)] for octaves 0..K: octave k is reduce2 of octave k - 1, values rounded to fp32 as the device stores them."""
    out = [(np.asarray(x, np.float32), mask)]
    for _ in range(K):
        v, clear, _ = reduce2(*out[-1])
        out.append((v.astype(np.float32), clear.astype(np.float32)))
    return out


def pyramid(ref, ref_mask, view, view_mask, octaves=2, P=7, levels=6, radius=4.0, coarse_levels=3, refine_radius=1.0):
    """-> (shift (2,) fp32 in pixels of the frame, trace (octaves + 1, 3) = (dy, dx, score) of every octave's last level in that
    octave's pixels, coarsest first).  Octave K from (0, 0) with `radius`, octave k < K from twice octave k + 1's shift with
    `refine_radius`; octave 0 takes `levels` levels, the others `coarse_levels`."""
    refs, views = octaves_of(ref, ref_mask, octaves), octaves_of(view, view_mask, octaves)
    shift = np.zeros(2, np.float32)
    trace = np.zeros((octaves + 1, 3))
    for k in range(octaves, -1, -1):
        top = k == octaves
        shift, t = search_from(refs[k][0], refs[k][1], views[k][0], views[k][1], (0.0, 0.0) if top else np.float32(2.0) * shift, P,
                               levels if k == 0 else coarse_levels, radius if top else refine_radius)
        trace[octaves - k] = t[-1]
    return shift, trace


def pad_for(shifts):
    """The pad of a scene whose views lie up to max |shift| apart: that many whole pixels and 10 more, so that nothing wraps around."""
    return int(np.ceil(np.abs(np.asarray(shifts)).max())) + 10


def scene(H, W, shifts, seed):
    """registration_ref.scene - the same spectrum, masks and noise - synthesised on a frame padded by pad_for(shifts) instead of
    registration_ref.PAD, which a shift of more than 8 pixels would wrap around."""
    keep = R.PAD
    R.PAD = pad_for(shifts)
    try:
        return R.scene(H, W, shifts, seed)
    finally:
        R.PAD = keep
