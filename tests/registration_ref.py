"""The masked-NCC registration search restated in numpy fp64, for the tests of hrnet_hip.registration, and the
synthetic scenes with known sub-pixel shifts those tests register.  Nothing here is taken from the reference fork's code: its method
(registration_search.py: a recursive grid search for the translation of maximal masked NCC) is restated on this project's own
definitions.  A shift s = (dy, dx) means Output(y, x) = Input(y + dy, x + dx), the convention of lanczos_shift.

Everything is float64 except what the definition fixes as float32: a grid coordinate is computed in fp64 and rounded to fp32, and its
split into the integer n = floor(d) and the fraction f = d - n is taken on that fp32 value (f itself is then exact in fp64).
No test logic here."""
import numpy as np

TAPS = np.arange(-2, 4)          # the six sample offsets o of the sampler


def split(d):
    """fp32 coordinate -> (n, f): n = floor(d) as an int, f = d - n in [0, 1) as an exact fp64."""
    d = np.float32(d)
    n = int(np.floor(np.float64(d)))
    return n, float(np.float64(d) - n)


def taps(f):
    """The six weights k_o = sinc(o - f) sinc((o - f) / 3), zero for |o - f| >= 3, normalised to sum 1."""
    x = TAPS - np.float64(f)
    k = np.sinc(x) * np.sinc(x / 3.0)
    k[np.abs(x) >= 3.0] = 0.0
    return k / k.sum()


def _axis(n, L):
    """The pixels of an axis of length L whose footprint p + n - 2 .. p + n + 3 lies inside it: [lo, hi)."""
    return max(0, 2 - n), min(L, L - 3 - n)


def inside(shape, shift):
    """(H, W) bool: the pixels whose 6 x 6 footprint lies inside the frame."""
    H, W = shape
    (ny, _), (nx, _) = split(shift[0]), split(shift[1])
    out = np.zeros((H, W), bool)
    (y0, y1), (x0, x1) = _axis(ny, H), _axis(nx, W)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = True
    return out


def sample(T, shift):
    """S(T, s): (H, W) float64, the taps applied along rows (dx) and then along columns (dy); 0 where the footprint leaves the frame."""
    T = np.asarray(T, np.float64)
    H, W = T.shape
    (ny, fy), (nx, fx) = split(shift[0]), split(shift[1])
    ky, kx = taps(fy), taps(fx)
    out = np.zeros((H, W))
    (y0, y1), (x0, x1) = _axis(ny, H), _axis(nx, W)
    if y0 >= y1 or x0 >= x1:
        return out
    A = np.zeros((H, x1 - x0))
    for o, k in zip(TAPS, kx):
        A += k * T[:, x0 + nx + o:x1 + nx + o]
    t = np.zeros((y1 - y0, x1 - x0))
    for o, k in zip(TAPS, ky):
        t += k * A[y0 + ny + o:y1 + ny + o]
    out[y0:y1, x0:x1] = t
    return out


def mask_bilinear(M, shift):
    """The bilinear sample of M at (y + dy, x + dx), zeros outside the frame: (H, W) float64."""
    M = np.asarray(M, np.float64)
    H, W = M.shape
    (ny, fy), (nx, fx) = split(shift[0]), split(shift[1])
    big = np.zeros((3 * H + 2, 3 * W + 2))
    big[H:2 * H, W:2 * W] = M

    def at(dy, dx):
        oy, ox = ny + dy, nx + dx
        if abs(oy) > H or abs(ox) > W:
            return np.zeros((H, W))
        return big[H + oy:2 * H + oy, W + ox:2 * W + ox]

    return (1.0 - fy) * ((1.0 - fx) * at(0, 0) + fx * at(0, 1)) + fy * ((1.0 - fx) * at(1, 0) + fx * at(1, 1))


def shifted_mask(M, shift):
    """V(M, s): (H, W) bool, the bilinear sample above 0.5 and the footprint inside the frame."""
    return (mask_bilinear(M, shift) > 0.5) & inside(np.shape(M), shift)


def score(ref, ref_mask, view, view_mask, shift):
    """The two-sided masked NCC of `ref` and S(view, shift) over c = ref_mask V(view_mask, shift); -inf without a pixel or a variance."""
    ref = np.asarray(ref, np.float64)
    rm = np.ones(ref.shape, bool) if ref_mask is None else np.asarray(ref_mask) != 0
    vm = np.ones(ref.shape) if view_mask is None else (np.asarray(view_mask) != 0).astype(np.float64)
    c = rm & shifted_mask(vm, shift)
    n = int(c.sum())
    if n == 0:
        return -np.inf
    t, r = sample(view, shift)[c], ref[c]
    t, r = t - t.mean(), r - r.mean()
    vt, vr = (t * t).sum() / n, (r * r).sum() / n
    if not (vt > 0.0 and vr > 0.0):
        return -np.inf
    return float((r * t).sum() / (n * np.sqrt(vr) * np.sqrt(vt)))


def grid_coords(c, width, P):
    """The P fp32 coordinates of a grid axis: c - w/2 + i w / (P - 1) in fp64, rounded to fp32."""
    c, w = np.float64(np.float32(c)), np.float64(width)
    return np.array([np.float32(c - w / 2.0 + i * w / (P - 1)) for i in range(P)], np.float32)


def grid(ref, ref_mask, view, view_mask, centre, width, P):
    """One grid level: -> (scores (P, P) float64 for (dy_i, dx_j), dys (P,) fp32, dxs (P,) fp32)."""
    dys, dxs = grid_coords(centre[0], width, P), grid_coords(centre[1], width, P)
    s = np.array([[score(ref, ref_mask, view, view_mask, (dy, dx)) for dx in dxs] for dy in dys])
    return s, dys, dxs


def best_of(scores, dys, dxs, centre):
    """The first maximum in row-major order (strict >); without a finite score the centre is kept and the score is -inf."""
    best, at = -np.inf, (np.float32(centre[0]), np.float32(centre[1]))
    for i in range(len(dys)):
        for j in range(len(dxs)):
            if scores[i, j] > best:
                best, at = scores[i, j], (dys[i], dxs[j])
    return at, best


def level_widths(P, levels, radius):
    """w_0 = 2 radius, w_{k+1} = w_k s in fp64, with s = 1 / (P - 2) raised to 0.25 if smaller and set to 0.9 if >= 1."""
    s = 1.0 / (P - 2)
    s = 0.9 if s >= 1.0 else max(s, 0.25)
    w, out = 2.0 * np.float64(np.float32(radius)), []
    for _ in range(levels):
        out.append(w)
        w = w * s
    return out


def search(ref, ref_mask, view, view_mask, P=7, levels=6, radius=1.0):
    """-> (shift (2,) fp32, trace (levels, 3) float64 = (dy, dx, score) of every level's best point)."""
    centre = (np.float32(0.0), np.float32(0.0))
    trace = np.zeros((levels, 3))
    for k, w in enumerate(level_widths(P, levels, radius)):
        s, dys, dxs = grid(ref, ref_mask, view, view_mask, centre, w, P)
        centre, best = best_of(s, dys, dxs, centre)
        trace[k] = (centre[0], centre[1], best)
    return np.array(centre, np.float32), trace


# ----------------------------------------------------------------------------- synthetic scenes with known shifts
PAD = 8                      # the frame is synthesised this much larger per side, so the crop has no wrap-around
LOWPASS_SIGMA = 0.12         # cycles / pixel


def _parts(H, W, shifts, seed):
    """What `scene` and `scene_stepped` are made of, drawn in one order: -> (z (H,W), z shifted per view, N(0, 1) per view, ref_mask,
    view_masks), float64 but the float32 masks."""
    rng = np.random.default_rng(seed)
    Hp, Wp = H + 2 * PAD, W + 2 * PAD
    ky, kx = np.fft.fftfreq(Hp)[:, None], np.fft.fftfreq(Wp)[None, :]
    F = np.fft.fft2(rng.standard_normal((Hp, Wp))) * np.exp(-(ky * ky + kx * kx) / (2.0 * LOWPASS_SIGMA ** 2))
    norm = np.fft.ifft2(F).real.std()

    def crop(ty, tx):
        z = np.fft.ifft2(F * np.exp(-2j * np.pi * (ky * ty + kx * tx))).real / norm
        return z[PAD:PAD + H, PAD:PAD + W]

    def mask():
        m = np.ones((H, W), np.float32)
        for _ in range(max(1, int(round(H * W / 400.0)))):
            cy, cx = rng.integers(0, H), rng.integers(0, W)
            hy, hx = rng.integers(2, 5, size=2)
            m[max(0, cy - hy):cy + hy + 1, max(0, cx - hx):cx + hx + 1] = 0.0
        return m

    z = crop(0.0, 0.0)
    ref_mask = mask()
    shifted, noise = [], []
    for ty, tx in shifts:
        shifted.append(crop(ty, tx))
        noise.append(rng.standard_normal((H, W)))
    view_masks = np.stack([mask() for _ in shifts])
    return z, shifted, noise, ref_mask, view_masks


def scene(H, W, shifts, seed):
    """A reference frame and len(shifts) templates of it: -> (ref (H,W), ref_mask (H,W), views (V,H,W), view_masks (V,H,W)), float32.
    White noise on a frame padded by PAD, a Gaussian low-pass in the FFT domain, the template at the sub-pixel offset (ty, tx) by a
    Fourier phase ramp - so that S(template, (ty, tx)) is the reference - then the crop; ref = 0.3 + 0.1 z, template = 0.32 + 0.11
    z_shifted + 0.002 N(0, 1); every mask has about one zero rectangle of half-sides 2..4 per 400 pixels."""
    z, shifted, noise, ref_mask, view_masks = _parts(H, W, shifts, seed)
    ref = (0.3 + 0.1 * z).astype(np.float32)
    views = np.stack([0.32 + 0.11 * zs + 0.002 * n for zs, n in zip(shifted, noise)]).astype(np.float32)
    return ref, ref_mask, views, view_masks


STEP_BAND = 6                # scene_stepped's band: this many pixels on either side of the step


def scene_stepped(H, W, shifts, seed, contrast, step, split, axis):
    """`scene`'s z, shifts, noise and speckle masks on a level with a step: -> (ref, ref_mask, views, view_masks, band), float32.
    ref = 0.2 + contrast z + step [p >= split], template = 0.2 + 1.1 contrast z_shifted + 0.002 (contrast / 0.1) N(0, 1) + step
    [p >= split], p the column (axis = 1) or the row (axis = 0): the level of either side is far from the frame's mean, the contrast may
    be small against both.  band (H,W) is zero on p = split - STEP_BAND .. split + STEP_BAND - 1 and one elsewhere: under it no pixel's
    6 x 6 footprint crosses the step for shifts within +-2 pixels."""
    z, shifted, noise, ref_mask, view_masks = _parts(H, W, shifts, seed)
    p = np.arange(W)[None, :] if axis == 1 else np.arange(H)[:, None]
    level = 0.2 + step * np.broadcast_to(p >= split, (H, W))
    ref = (level + contrast * z).astype(np.float32)
    views = np.stack([level + 1.1 * contrast * zs + 0.002 * (contrast / 0.1) * n for zs, n in zip(shifted, noise)]).astype(np.float32)
    band = np.broadcast_to((p < split - STEP_BAND) | (p >= split + STEP_BAND), (H, W)).astype(np.float32)
    return ref, ref_mask, views, view_masks, band


def random_shifts(V, limit, seed):
    """(V, 2) true shifts, uniform in +-limit."""
    return np.random.default_rng(seed).uniform(-limit, limit, size=(V, 2))
