"""The backward of the six-tap sampler restated in numpy fp64, for the tests of hrnet_hip.registration.warp and
hrn_mncc_apply_backward.  Built on registration_ref: split, taps, _axis, inside and sample are its own.  With (n, f) = split(d) per axis
and k = taps(f):

    g          = d_out where `valid` is non-zero and the pixel's 6 x 6 footprint lies inside the frame, else 0
    d_views    (p, q) = sum_{a, b = -2..3} k^y_a k^x_b g(p - n_y - a, q - n_x - b), g zero outside the frame
    d_shifts   [0] = sum_pixels g dS/ddy,  dS/ddy = S with k'^y in place of k^y;  [1] the mirror
    k'_o       = (u'_o - k_o sum u') / sum u,  u_o = L3(o - f),  u'_o = -L3'(o - f),  L3(t) = sinc(t) sinc(t / 3) inside |t| < 3

The keyword arguments of d_views, dtaps and d_shifts exist for the tests' controls: each turns one part of the definition into the
mistake that part guards against.  No test logic here."""
import numpy as np

import registration_ref as R

# the shifts every shape of tests/test_gpu_warp.py meets (its docstring says what each is for); tests/test_gpu_large_offsets_scene.py cycles
# through them too
SHIFTS = [(0.37, -0.62), (2.0, 0.0), (0.0, 0.0), (-3.75, 4.125), (0.9999999, -1e-7), (30.0, 0.0), (300.0, 0.0)]


def _sinc_slope(t):
    """sinc'(t) for sinc(t) = sin(pi t) / (pi t).  The closed form (cos(pi t) - sinc(t)) / t cancels near 0: below 1e-2 the series
    pi (-z / 3 + z^3 / 30 - z^5 / 840), z = pi t, whose first dropped term is below 3e-15 there."""
    t = np.asarray(t, np.float64)
    z = np.pi * t
    small = np.abs(t) < 1e-2
    closed = (np.cos(z) - np.sinc(t)) / np.where(small, 1.0, t)
    return np.where(small, np.pi * z * (-1.0 / 3.0 + z * z * (1.0 / 30.0 - z * z / 840.0)), closed)


def dtaps(f, normalise=True):
    """The six derivatives k'_o = d k_o / d f of taps(f).  normalise=False drops the term of the normalisation, k_o sum u' / sum u."""
    x = R.TAPS - np.float64(f)
    a, b = np.sinc(x), np.sinc(x / 3.0)
    u = a * b
    du = -(_sinc_slope(x) * b + a * _sinc_slope(x / 3.0) / 3.0)
    u[np.abs(x) >= 3.0] = 0.0
    du[np.abs(x) >= 3.0] = 0.0
    if not normalise:
        return du / u.sum()
    return (du - (u / u.sum()) * du.sum()) / u.sum()


def _apply(T, shift, ky, kx):
    """registration_ref.sample with the taps given: kx along rows at the whole part n_x, then ky along columns at n_y; 0 where the
    footprint leaves the frame."""
    T = np.asarray(T, np.float64)
    H, W = T.shape
    (ny, _), (nx, _) = R.split(shift[0]), R.split(shift[1])
    out = np.zeros((H, W))
    (y0, y1), (x0, x1) = R._axis(ny, H), R._axis(nx, W)
    if y0 >= y1 or x0 >= x1:
        return out
    A = np.zeros((H, x1 - x0))
    for o, k in zip(R.TAPS, kx):
        A += k * T[:, x0 + nx + o:x1 + nx + o]
    t = np.zeros((y1 - y0, x1 - x0))
    for o, k in zip(R.TAPS, ky):
        t += k * A[y0 + ny + o:y1 + ny + o]
    out[y0:y1, x0:x1] = t
    return out


def _fracs(shift):
    return R.split(shift[0])[1], R.split(shift[1])[1]


def sample_d(T, shift):
    """-> (S, dS/ddy, dS/ddx), each (H, W) float64 and 0 where the footprint leaves the frame."""
    fy, fx = _fracs(shift)
    ky, kx = R.taps(fy), R.taps(fx)
    return R.sample(T, shift), _apply(T, shift, dtaps(fy), kx), _apply(T, shift, ky, dtaps(fx))


def masked(d_out, valid, shift):
    """g: d_out where valid is non-zero and the footprint lies inside the frame, else 0."""
    d_out = np.asarray(d_out, np.float64)
    return np.where((np.asarray(valid) != 0) & R.inside(d_out.shape, shift), d_out, 0.0)


def _moved(Z, dy, dx):
    """M(p, q) = Z(p + dy, q + dx), zero outside the frame."""
    H, W = Z.shape
    out = np.zeros((H, W))
    p0, p1, q0, q1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    if p0 < p1 and q0 < q1:
        out[p0:p1, q0:q1] = Z[p0 + dy:p1 + dy, q0 + dx:q1 + dx]
    return out


def _gather(Z, shift, ky, kx, reverse=True, whole=-1):
    """The sampler's two passes over Z with the taps reversed, the whole parts (-n_y + whole, -n_x + whole) and zero padding."""
    (ny, _), (nx, _) = R.split(shift[0]), R.split(shift[1])
    if reverse:
        ky, kx = ky[::-1], kx[::-1]
    out = np.zeros(Z.shape)
    for oy, a in zip(R.TAPS, ky):
        for ox, b in zip(R.TAPS, kx):
            out += a * b * _moved(Z, -ny + whole + int(oy), -nx + whole + int(ox))
    return out


def d_views(d_out, valid, shift, reverse=True, whole=-1):
    """The gradient of sum(d_out * S(T, shift)) over the valid pixels with respect to T, in the gather form: (H, W) float64.  Tap index m
    of the reversed taps multiplies g(p - n_y - 1 + m - 2), which is k_a g(p - n_y - a) for a = 3 - m."""
    fy, fx = _fracs(shift)
    return _gather(masked(d_out, valid, shift), shift, R.taps(fy), R.taps(fx), reverse, whole)


def d_shifts(T, d_out, valid, shift, slope=dtaps):
    """The gradient of the same sum with respect to (dy, dx): (2,) float64.  slope: what stands for k'."""
    fy, fx = _fracs(shift)
    g = masked(d_out, valid, shift)
    return np.array([(g * _apply(T, shift, slope(fy), R.taps(fx))).sum(), (g * _apply(T, shift, R.taps(fy), slope(fx))).sum()])


def magnitudes(T, d_out, valid, shift):
    """The same sums over absolute values, the T of kernel_bounds._bound: -> (for d_views (H, W), for d_shifts (2,))."""
    fy, fx = _fracs(shift)
    ky, kx, dy, dx = np.abs(R.taps(fy)), np.abs(R.taps(fx)), np.abs(dtaps(fy)), np.abs(dtaps(fx))
    g, A = np.abs(masked(d_out, valid, shift)), np.abs(np.asarray(T, np.float64))
    return _gather(g, shift, ky, kx), np.array([(g * _apply(A, shift, dy, kx)).sum(), (g * _apply(A, shift, ky, dx)).sum()])
