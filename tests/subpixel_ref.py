"""The sub-pixel searched cMSE / cPSNR loss (include/hrnet_hip.h) restated in numpy fp64, in the DIRECT form: the
residual image is formed and squared, nothing goes through the six sums the kernels keep (`six_sums` is that formula, for the test that
the two agree).  Built on registration_ref (sample, inside, grid_coords, level_widths, best_of) and warp_ref.d_views.

A shift s = (dy, dx) means S(sr, s)(p) = sr(p + s).  For one sample
    m0 = (hr_map != 0) and p at least `border` from every frame edge;  c(s) = m0 and the 6 x 6 footprint of p at s inside the frame
    n = |c|,  b = mean over c of (hr - S(sr, s)),  e = S(sr, s) + b - hr,  cMSE = mean over c of e^2
    the search: `levels` grids of P x P points around the previous best, the first around (0, 0) with width 2 radius; the best point is
    the first maximum of -cMSE in row-major order (strict), -inf where n = 0
    the gradient with s* held: g = d_out factor 2 c e / n (factor 1 for cMSE, -10 / (ln 10 cMSE) for cPSNR), d_sr = the sampler's adjoint

The keyword arguments named in CONTROLS exist for the tests' controls: each turns one part of the definition into the mistake that part
guards against.  No test logic here."""
import numpy as np

import registration_ref as R
import warp_ref

CONTROLS = ("no_bias", "no_crop", "no_footprint", "taps_not_reversed", "n_of_centre", "no_cpsnr_factor")
SHAPES = [((24, 40), 1), ((70, 83), 2), ((130, 203), 3)]                     # (H, W), seed: the issue's scenes
SHIFTS = [(0.37, -0.62), (2.0, 0.0), (-2.4, 1.55), (0.0, 0.0), (2.9, -2.9)]
P, LEVELS, RADIUS, BORDER = 7, 4, 3.0, 3
LAST_STEP = 2 * RADIUS * 0.25 ** (LEVELS - 1) / (P - 1)                     # 0.015625 px


def scene(H, W, shift, seed):
    """-> (sr, hr, hr_map) float32: hr = 0.3 + 0.1 z, sr = 0.33 + 0.1 z_shifted + 0.002 N, so that S(sr, shift) is hr up to the noise and
    the brightness; hr_map = the speckle mask of registration_ref's scenes."""
    z, shifted, noise, ref_mask, _ = R._parts(H, W, [shift], seed)
    return (0.33 + 0.1 * shifted[0] + 0.002 * noise[0]).astype(np.float32), (0.3 + 0.1 * z).astype(np.float32), ref_mask


def crop_mask(hr_map, border, no_crop=False):
    m = np.asarray(hr_map) != 0
    if border > 0 and not no_crop:
        inner = np.zeros_like(m)
        inner[border:m.shape[0] - border, border:m.shape[1] - border] = True
        m = m & inner
    return m


def residual(sr, hr, hr_map, border, shift, no_bias=False, no_crop=False, no_footprint=False):
    """-> (c (H,W) bool, n, b, e (H,W) = S(sr, s) + b - hr, zero off c).  n = 0: b = 0 and e = 0."""
    hr = np.asarray(hr, np.float64)
    c = crop_mask(hr_map, border, no_crop)
    if not no_footprint:
        c = c & R.inside(hr.shape, shift)
    n = int(c.sum())
    if n == 0:
        return c, 0, 0.0, np.zeros(hr.shape)
    t = R.sample(sr, shift)
    b = 0.0 if no_bias else float((hr - t)[c].sum() / n)
    return c, n, b, np.where(c, t + b - hr, 0.0)


def cmse(sr, hr, hr_map, border, shift, **kw):
    """-> (cMSE, n, b); cMSE = inf where n = 0"""
    c, n, b, e = residual(sr, hr, hr_map, border, shift, **kw)
    return (float((e * e).sum() / n) if n else np.inf), n, b


def six_sums(sr, hr, hr_map, border, shift, mean_sr=0.0, mean_hr=0.0, dtype=np.longdouble):
    """the kernels' formula: the six sums over c of t = S(sr - mean_sr, s) and r = hr - mean_hr -> (cMSE, the centred bias, n).  The sums
    and the formula are evaluated in `dtype`.  In float64 the last step cancels sums of magnitude n var down to n cMSE, which costs about
    2^-52 var / cMSE relative - 1e-12 where var / cMSE = 4e3 - so the identity itself is checked in long double."""
    c, n, _, _ = residual(sr, hr, hr_map, border, shift)
    t = R.sample(np.asarray(sr, np.float64) - mean_sr, shift)[c].astype(dtype)
    r = (np.asarray(hr, np.float64) - mean_hr)[c].astype(dtype)
    st, sr_, stt, srr, srt = t.sum(), r.sum(), (t * t).sum(), (r * r).sum(), (r * t).sum()
    return float(max(0.0, (stt + srr - 2 * srt - (st - sr_) ** 2 / n) / n)), float((sr_ - st) / n), n


def magnitude(sr, shift):
    """T of the sampler: sum |k| |sr| over the footprint, (H,W); kernel_bounds' T for S(sr, s)"""
    fy, fx = warp_ref._fracs(shift)
    return warp_ref._apply(np.abs(np.asarray(sr, np.float64)), shift, np.abs(R.taps(fy)), np.abs(R.taps(fx)))


def cmse_bound(sr, hr, hr_map, border, shift, C, **kw):
    """|device cMSE - fp64 cMSE| at one point, from the sampler's fp32 error delta_p = C T_p per pixel carried through the square:
    2 mean(|e| delta) + mean(delta^2) (the bias correction only takes the mean of the error off), plus the fp64 rounding of the six
    sums, 4 n 2^-53 (mean t^2 + mean r^2), on images centred by their means.  inf where n = 0 (nothing to compare)."""
    c, n, b, e = residual(sr, hr, hr_map, border, shift, **kw)
    if n == 0:
        return np.inf
    d = C * magnitude(sr, shift)[c]
    t, r = R.sample(sr, shift)[c], np.asarray(hr, np.float64)[c]
    centred = ((t - t.mean()) ** 2).mean() + ((r - r.mean()) ** 2).mean()
    return float(2.0 * (np.abs(e[c]) * d).mean() + (d * d).mean() + 4.0 * n * 2.0 ** -53 * centred)


def search(sr, hr, hr_map, border=BORDER, P=P, levels=LEVELS, radius=RADIUS, **kw):
    """-> dict: shift (2,) fp32 s*, trace (levels,3) = (dy, dx, cMSE), scores (levels,P,P) cMSE (inf where n = 0), coords (levels,2,P)
    fp32, gaps (levels,) the relative gap between the lowest and the second-lowest cMSE of a level, n, b, cmse at s* (n = 0: cmse NaN)."""
    centre = (np.float32(0.0), np.float32(0.0))
    trace, scores, coords, gaps = np.zeros((levels, 3)), np.zeros((levels, P, P)), np.zeros((levels, 2, P), np.float32), np.zeros(levels)
    n = b = 0
    for k, w in enumerate(R.level_widths(P, levels, radius)):
        dys, dxs = R.grid_coords(centre[0], w, P), R.grid_coords(centre[1], w, P)
        got = [[cmse(sr, hr, hr_map, border, (dy, dx), **kw) for dx in dxs] for dy in dys]
        s = np.array([[g[0] for g in row] for row in got])
        centre, best = R.best_of(-s, dys, dxs, centre)
        scores[k], coords[k, 0], coords[k, 1] = s, dys, dxs
        two = np.sort(s.ravel())[:2]
        gaps[k] = (two[1] - two[0]) / two[0] if np.isfinite(two[1]) and two[0] > 0 else np.inf
        value = -best if np.isfinite(best) else np.nan
        trace[k] = (centre[0], centre[1], value)
        if k == levels - 1 and np.isfinite(best):
            i, j = int(np.argmax(dys == centre[0])), int(np.argmax(dxs == centre[1]))
            n, b = got[i][j][1], got[i][j][2]
    return dict(shift=np.array(centre, np.float32), trace=trace, scores=scores, coords=coords, gaps=gaps, n=n, b=b, cmse=trace[-1, 2])


def loss_of(value, metric):
    return -10.0 * np.log10(value) if metric == "cPSNR" else value


def grad(sr, hr, hr_map, border, shift, metric, d_out=1.0, no_bias=False, no_crop=False, no_footprint=False, taps_not_reversed=False,
         n_of_centre=False, no_cpsnr_factor=False):
    """d loss / d sr with the shift held: (H,W) float64, every element defined, zero where no counted pixel's footprint reaches"""
    c, n, b, e = residual(sr, hr, hr_map, border, shift, no_bias, no_crop, no_footprint)
    if n == 0:
        return np.zeros(np.shape(hr))
    value = float((e * e).sum() / n)
    factor = -10.0 / (np.log(10.0) * value) if metric == "cPSNR" and not no_cpsnr_factor else 1.0
    if n_of_centre:
        n = residual(sr, hr, hr_map, border, (0.0, 0.0), no_bias, no_crop, no_footprint)[1]
    g = d_out * factor * 2.0 * e / n
    return warp_ref.d_views(g, c, shift, reverse=not taps_not_reversed)


def grad_magnitude(sr, hr, hr_map, border, shift, metric, d_out, C):
    """T of d_sr per element, for |got - want| <= C T.  A counted pixel's residual carries the sampler's error C (T_p + mean T) (its own
    and the bias's), g = coef e is rounded to fp32 and goes through the adjoint's fp32 passes: T = sum |k| |coef| (|e| + T_p + mean T).
    For cPSNR the factor is formed from the device's own cMSE*, whose relative error is at most rel = B / (cMSE - B) with B =
    cmse_bound: that adds sum |k| |coef| |e| rel / C."""
    c, n, b, e = residual(sr, hr, hr_map, border, shift)
    if n == 0:
        return np.zeros(np.shape(hr))
    value = float((e * e).sum() / n)
    coef = abs(d_out) * 2.0 / n * (10.0 / (np.log(10.0) * value) if metric == "cPSNR" else 1.0)
    Tp = magnitude(sr, shift)
    fy, fx = warp_ref._fracs(shift)
    ky, kx = np.abs(R.taps(fy)), np.abs(R.taps(fx))
    per_pixel = np.where(c, coef * (np.abs(e) + Tp + Tp[c].mean()), 0.0)
    T = warp_ref._gather(per_pixel, shift, ky, kx)
    if metric == "cPSNR":
        B = cmse_bound(sr, hr, hr_map, border, shift, C)
        rel = B / (value - B) if value > B else np.inf
        T = T + warp_ref._gather(np.where(c, coef * np.abs(e), 0.0), shift, ky, kx) * (rel / C)
    return T
