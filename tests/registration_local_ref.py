"""The shift field of a scene restated in numpy fp64, for the tests of hrnet_hip.registration's mncc_search_local /
shift_field: the blocks of an axis and their nodes, the score of a block (tests/registration_ref.py's score with the reference mask set
to zero outside the block), the search per block, the field at every pixel, the sampler and the valid map pixel by pixel, and a scene
warped by a known field.  Everything is float64 except what the definitions fix as float32: a grid coordinate, and the field at a
pixel after its fp64 interpolation.  No test logic here."""
import numpy as np

import registration_ref as R


# ----------------------------------------------------------------------------- blocks and nodes
def blocks(L, block):
    """The number of blocks of an axis of length L."""
    return max(1, (L + block // 2) // block)


def bounds(L, block):
    """[(r0, r1)] of the blocks of an axis: block i covers [i block, (i + 1) block), the last one runs to L."""
    n = blocks(L, block)
    return [(i * block, L if i == n - 1 else (i + 1) * block) for i in range(n)]


def nodes(L, block):
    """The centre (r0 + r1 - 1) / 2 of every block of an axis, float64."""
    return np.array([(r0 + r1 - 1) / 2.0 for r0, r1 in bounds(L, block)])


def restricted(ref_mask, shape, rows, cols):
    """The reference mask (None: all clear) set to zero outside rows [r0, r1) x cols [c0, c1): float32."""
    out = np.zeros(shape, np.float32)
    sl = (slice(*rows), slice(*cols))
    out[sl] = 1.0 if ref_mask is None else (np.asarray(ref_mask)[sl] != 0)
    return out


def block_score(ref, ref_mask, view, view_mask, shift, rows, cols):
    """The local score of the block rows x cols at `shift`."""
    return R.score(ref, restricted(ref_mask, np.shape(ref), rows, cols), view, view_mask, shift)


def common_valid(ref_mask, view_mask, shape, shift, rows, cols):
    """n: the pixels of the block that are clear in the reference and valid in the view resampled by `shift`."""
    vm = np.ones(shape) if view_mask is None else (np.asarray(view_mask) != 0).astype(np.float64)
    return int(((restricted(ref_mask, shape, rows, cols) != 0) & R.shifted_mask(vm, shift)).sum())


# ----------------------------------------------------------------------------- the search per block
def search_local(ref, ref_mask, view, view_mask, block, init=None, P=7, levels=4, radius=0.5, min_valid=0.25):
    """-> (field (by, bx, 2) fp32, trace (by, bx, levels, 3) float64, ok (by, bx) bool, n (by, bx) int at the last chosen point)."""
    H, W = np.shape(ref)
    rows, cols = bounds(H, block), bounds(W, block)
    start = (np.float32(0.0), np.float32(0.0)) if init is None else (np.float32(init[0]), np.float32(init[1]))
    field = np.zeros((len(rows), len(cols), 2), np.float32)
    trace = np.zeros((len(rows), len(cols), levels, 3))
    ok, count = np.zeros((len(rows), len(cols)), bool), np.zeros((len(rows), len(cols)), np.int64)
    for i, rr in enumerate(rows):
        for j, cc in enumerate(cols):
            rm = restricted(ref_mask, (H, W), rr, cc)
            centre, best = start, -np.inf
            for k, w in enumerate(R.level_widths(P, levels, radius)):
                s, dys, dxs = R.grid(ref, rm, view, view_mask, centre, w, P)
                centre, best = R.best_of(s, dys, dxs, centre)
                trace[i, j, k] = (centre[0], centre[1], best)
            count[i, j] = common_valid(ref_mask, view_mask, (H, W), centre, rr, cc)
            area = np.float64((rr[1] - rr[0]) * (cc[1] - cc[0]))
            ok[i, j] = bool(np.isfinite(best) and np.float64(count[i, j]) >= np.float64(np.float32(min_valid)) * area)
            field[i, j] = centre if ok[i, j] else start
    return field, trace, ok, count


# ----------------------------------------------------------------------------- the field at a pixel
def axis_weights(L, block):
    """Per pixel of an axis: (k, k + 1 or k with one block, t) - the last node at or before the pixel within [0, n - 2], and
    t = clamp((p - node_k) / (node_{k+1} - node_k), 0, 1); with one block k = 0 and t = 0."""
    nd, p = nodes(L, block), np.arange(L, dtype=np.float64)
    if len(nd) < 2:
        return np.zeros(L, np.int64), np.zeros(L, np.int64), np.zeros(L)
    k = np.clip(np.searchsorted(nd, p, side="right") - 1, 0, len(nd) - 2)
    t = np.clip((p - nd[k]) / (nd[k + 1] - nd[k]), 0.0, 1.0)
    return k, k + 1, t


def field_at_pixels(field, H, W, block, rounded=True, rows=None):
    """field (by, bx, 2) -> (H, W, 2): (1 - ty) ((1 - tx) N00 + tx N01) + ty ((1 - tx) N10 + tx N11) in fp64, in this order; rounded to
    fp32 as a grid coordinate is (rounded=False: the fp64 values).  rows = (a, b): only the frame's rows a .. b - 1, (b - a, W, 2)."""
    N = np.asarray(field, np.float32).astype(np.float64)
    ky, ky1, ty = (w[slice(*rows)] if rows is not None else w for w in axis_weights(H, block))
    kx, kx1, tx = axis_weights(W, block)
    ty, tx = ty[:, None, None], tx[None, :, None]
    n00, n01 = N[ky[:, None], kx[None, :]], N[ky[:, None], kx1[None, :]]
    n10, n11 = N[ky1[:, None], kx[None, :]], N[ky1[:, None], kx1[None, :]]
    out = (1.0 - ty) * ((1.0 - tx) * n00 + tx * n01) + ty * ((1.0 - tx) * n10 + tx * n11)
    return out.astype(np.float32) if rounded else out


# ----------------------------------------------------------------------------- the sampler and the valid map, pixel by pixel
def _split(d):
    d = np.asarray(d, np.float32).astype(np.float64)
    n = np.floor(d)
    return n.astype(np.int64), d - n


def _taps(f):
    x = R.TAPS[None, None, :] - f[..., None]
    k = np.sinc(x) * np.sinc(x / 3.0)
    k[np.abs(x) >= 3.0] = 0.0
    return k / k.sum(-1, keepdims=True)


def sample_field(T, M, shifts):
    """Every pixel of T (H, W) resampled by its own fp32 shift shifts[y, x] = (dy, dx), M (H, W) the mask or None: -> (out (H, W)
    float64, valid (H, W) bool, the bilinear mask sample (H, W) float64).  The six taps along the row for each of the six rows, then the
    six down the column.  A pixel is valid when its own footprint lies inside the frame and its own mask sample exceeds 0.5; the rest
    are 0."""
    T = np.asarray(T, np.float64)
    H, W = T.shape
    M = np.ones((H, W)) if M is None else (np.asarray(M) != 0).astype(np.float64)
    (ny, fy), (nx, fx) = _split(shifts[..., 0]), _split(shifts[..., 1])
    y, x = np.arange(H)[:, None] + ny, np.arange(W)[None, :] + nx
    inside = (y - 2 >= 0) & (y + 3 <= H - 1) & (x - 2 >= 0) & (x + 3 <= W - 1)
    rows = np.clip(y[..., None] + R.TAPS, 0, H - 1)
    cols = np.clip(x[..., None] + R.TAPS, 0, W - 1)
    window = T[rows[:, :, :, None], cols[:, :, None, :]]                     # (H, W, row of the footprint, column of the footprint)
    A = (window * _taps(fx)[:, :, None, :]).sum(-1)
    out = (A * _taps(fy)).sum(-1)
    big = np.zeros((H + 2, W + 2))
    big[:H, :W] = M

    def at(dy, dx):                                                          # the mask at (y + dy, x + dx), zero outside the frame
        yy, xx = y + dy, x + dx
        off = (yy < 0) | (yy > H) | (xx < 0) | (xx > W)
        return np.where(off, 0.0, big[np.clip(yy, 0, H), np.clip(xx, 0, W)])

    bil = (1.0 - fy) * ((1.0 - fx) * at(0, 0) + fx * at(0, 1)) + fy * ((1.0 - fx) * at(1, 0) + fx * at(1, 1))
    valid = inside & (bil > 0.5)
    return np.where(valid, out, 0.0), valid, bil


# ----------------------------------------------------------------------------- a scene warped by a known field
def linear_field(H, W):
    """The field of the recovery tests: t(y, x) = (0.2 + 0.5 (x / W - 0.5), -0.3 + 0.6 (y / H - 0.5)), at float positions."""
    return lambda y, x: (0.2 + 0.5 * (x / W - 0.5), -0.3 + 0.6 * (y / H - 0.5))


def recovered(t, y, x, iterations=30):
    """The shift a perfect registration finds at the positions (y, x): the fixed point s = t(p + s) - S(template, s)(p) = template(p + s)
    = ref(p + s - t(p + s)).  -> (..., 2) float64"""
    y, x = np.broadcast_arrays(np.asarray(y, np.float64), np.asarray(x, np.float64))
    sy, sx = np.zeros(y.shape), np.zeros(y.shape)
    for _ in range(iterations):
        sy, sx = t(y + sy, x + sx)
    return np.stack([sy, sx], -1)


def warped_scene(H, W, fields, seed):
    """registration_ref.scene with every template warped instead of shifted: template(q) = z(q - t(q)) for t in `fields`, z the same
    band-limited frame (white noise on a frame padded by PAD, the Gaussian low-pass of LOWPASS_SIGMA), evaluated off the pixel raster by
    the direct trigonometric sum over its spectrum.  -> (ref, ref_mask, views, view_masks) float32, as registration_ref.scene."""
    rng = np.random.default_rng(seed)
    Hp, Wp = H + 2 * R.PAD, W + 2 * R.PAD
    ky, kx = np.fft.fftfreq(Hp), np.fft.fftfreq(Wp)
    F = np.fft.fft2(rng.standard_normal((Hp, Wp))) * np.exp(-(ky[:, None] ** 2 + kx[None, :] ** 2) / (2.0 * R.LOWPASS_SIGMA ** 2))
    z0 = np.fft.ifft2(F).real
    norm = z0.std()

    def at(yy, xx):                                                          # z at the float positions (yy, xx) of the padded frame
        ey = np.exp(2j * np.pi * yy.reshape(-1, 1) * ky[None, :])            # (pixels, Hp)
        ex = np.exp(2j * np.pi * xx.reshape(-1, 1) * kx[None, :])            # (pixels, Wp)
        return ((ey @ F) * ex).sum(-1).real.reshape(yy.shape) / (Hp * Wp * norm)

    def mask():
        m = np.ones((H, W), np.float32)
        for _ in range(max(1, int(round(H * W / 400.0)))):
            cy, cx = rng.integers(0, H), rng.integers(0, W)
            hy, hx = rng.integers(2, 5, size=2)
            m[max(0, cy - hy):cy + hy + 1, max(0, cx - hx):cx + hx + 1] = 0.0
        return m

    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ref = (0.3 + 0.1 * z0[R.PAD:R.PAD + H, R.PAD:R.PAD + W] / norm).astype(np.float32)
    ref_mask = mask()
    views = []
    for t in fields:
        ty, tx = t(y, x)
        views.append(0.32 + 0.11 * at(y - ty + R.PAD, x - tx + R.PAD) + 0.002 * rng.standard_normal((H, W)))
    view_masks = np.stack([mask() for _ in fields])
    return ref, ref_mask, np.stack(views).astype(np.float32), view_masks


# ----------------------------------------------------------------------------- blocks that must fall back
FALLBACK_SHAPE, FALLBACK_BLOCK, FALLBACK_INIT = (70, 140), 64, (0.25, -0.5)      # 1 x 2 blocks: columns [0, 64) and [64, 140)


def fallback_cases(seed=5):
    """Two views of one scene (true shifts FALLBACK_INIT) whose block (0, 0) cannot be trusted: view 0 is masked over the whole block
    and a margin around it, view 1 keeps a 21 x 21 patch of it clear - 441 of the block's 70 x 64 = 4480 pixels, 10 %.  Block (0, 1) is
    as registration_ref.scene made it.  -> (ref, ref_mask, views (2, H, W), view_masks (2, H, W)) float32"""
    H, W = FALLBACK_SHAPE
    ref, ref_mask, views, view_masks = R.scene(H, W, [FALLBACK_INIT, FALLBACK_INIT], seed)
    view_masks = view_masks.copy()
    view_masks[:, :, :70] = 0.0
    view_masks[1, 20:41, 22:43] = 1.0
    return ref, ref_mask, views, view_masks
