"""Tiled inference (HRNet.forward_tiled): the window rule.  Pure Python / torch indexing, no GPU and no native library:
this module states the rule that hrn_tile_gather / hrn_tile_scatter restate on the device (csrc/tile.hip computes the same
geometry from (H, W, t, R, window index)), and it is the reference their tests compare against, bit for bit.

Why exact tiling is possible.  Every layer of HRNet is a zero-padded 3x3 convolution or acts per pixel (the median reference frame,
PReLU, the alpha residual, the non-overlapping stride-S deconvolution, the 1x1 final conv), so an SR pixel depends only on the LR
pixels within

    R = halo(num_layers, V) = 2 + 2 * num_layers + 3 * floor(log2 V)

LR pixels of its own LR pixel: the stem conv, two convs per encoder ResidualBlock, the encoder's final conv, and three convs for each
of the floor(log2 V) fusion levels.  A square window of side t therefore predicts a pixel exactly as the whole frame does if every
side of the window either LIES ON the scene's border (the network pads there, as it does for the whole frame) or is at least R pixels
away from that pixel.  A window that hangs over the border and is zero-filled is NOT equivalent: the network pads every layer, not
the input.  So every window lies inside the scene, and the last window of an axis is pulled back to end on the border.

Along one axis of length L >= t, with k = t - 2R: window 0 has core_lo = 0, window i >= 1 has core_lo = (t - R) + (i - 1) * k;

    start   = min(max(core_lo - R, 0), L - t)
    core_hi = L  if start + t == L  else  start + t - R

and the plan ends with the window whose core_hi == L.  The cores [core_lo, core_hi) partition [0, L); a window is responsible for
its core only.  A scene's plan is the row-major product of its two axis plans with t = min(tile, H, W): the windows are square
whatever the scene's shape, which is what lifts the forward's square-only limit.  The price is the overhead factor
n_windows * t * t / (H * W): pixels computed per pixel kept, -> (t / (t - 2R))^2 for large scenes."""
import collections

Window = collections.namedtuple("Window", "y0 x0 cy0 cy1 cx0 cx1")      # origin of the t x t window; its core [cy0, cy1) x [cx0, cx1)
Plan = collections.namedtuple("Plan", "H W t R ny nx windows overhead")  # windows: row-major list of ny * nx Window


def halo(num_layers, n_views):
    """The network's one-sided receptive field in LR pixels: 2 + 2 * num_layers + 3 * floor(log2(n_views))."""
    num_layers, n_views = int(num_layers), int(n_views)
    if num_layers < 0 or n_views < 1:
        raise ValueError(f"halo needs num_layers >= 0 and n_views >= 1, got {num_layers} and {n_views}")
    return 2 + 2 * num_layers + 3 * (n_views.bit_length() - 1)


def axis_count(L, t, R):
    """Closed form of len(axis_plan(L, t, R)): 1 if L == t, else ceil((L - 2R) / (t - 2R))."""
    if L == t:
        return 1
    k = t - 2 * R
    return -((2 * R - L) // k)


def _check_axis(L, t, R):
    if not (isinstance(L, int) and isinstance(t, int) and isinstance(R, int)) or R < 0 or t < 1 or L < t:
        raise ValueError(f"an axis plan needs integers L >= t >= 1 and R >= 0, got L={L!r} t={t!r} R={R!r}")
    if L > t and t < 2 * R + 1:
        raise ValueError(f"L={L} needs more than one window of t={t}, which must be at least 2R+1 = {2 * R + 1} (R={R})")


def axis_plan(L, t, R):
    """[(start, core_lo, core_hi), ...] along one axis of length L >= t (module docstring)."""
    _check_axis(L, t, R)
    k = t - 2 * R
    out, i = [], 0
    while True:
        core_lo = 0 if i == 0 else (t - R) + (i - 1) * k
        start = min(max(core_lo - R, 0), L - t)
        core_hi = L if start + t == L else start + t - R
        out.append((start, core_lo, core_hi))
        if core_hi == L:
            return out
        i += 1


def plan(H, W, tile, R):
    """The windows of an (H, W) scene for square windows of side t = min(tile, H, W): Plan(H, W, t, R, ny, nx, windows, overhead).
    ValueError naming H, W, tile and R when t < 2R + 1 while some axis needs more than one window; a single window (H == W == t) is
    always allowed."""
    if not all(isinstance(v, int) for v in (H, W, tile, R)) or H < 1 or W < 1 or tile < 1 or R < 0:
        raise ValueError(f"plan needs integers H, W, tile >= 1 and R >= 0, got H={H!r} W={W!r} tile={tile!r} R={R!r}")
    t = min(tile, H, W)
    if (H > t or W > t) and t < 2 * R + 1:
        raise ValueError(f"H={H} W={W} tile={tile} R={R}: the scene needs more than one window of side {t}, and a window that has a "
                         f"neighbour must be at least 2R+1 = {2 * R + 1} pixels wide to have a core")
    rows, cols = axis_plan(H, t, R), axis_plan(W, t, R)
    windows = [Window(y0, x0, cy0, cy1, cx0, cx1) for y0, cy0, cy1 in rows for x0, cx0, cx1 in cols]
    return Plan(H, W, t, R, len(rows), len(cols), windows, len(windows) * t * t / (H * W))


def gather(lrs, windows, t):
    """lrs (..., H, W) -> (n, ..., t, t), window-major: out[i] = lrs[..., y0 : y0 + t, x0 : x0 + t] of windows[i].  The rule of
    hrn_tile_gather."""
    import torch
    return torch.stack([lrs[..., w.y0:w.y0 + t, w.x0:w.x0 + t] for w in windows])


def scatter(out, srs, windows, t, scale):
    """srs (n, ..., S t, S t) -> the cores of `windows` in out (..., S H, S W), in place; nothing else of `out` is touched.  The rule
    of hrn_tile_scatter.  Returns `out`."""
    S = scale
    if len(srs) != len(windows) or tuple(srs.shape[-2:]) != (S * t, S * t):
        raise ValueError(f"srs must be ({len(windows)}, ..., {S * t}, {S * t}), got {tuple(srs.shape)}")
    for sr, w in zip(srs, windows):
        out[..., S * w.cy0:S * w.cy1, S * w.cx0:S * w.cx1] = sr[..., S * (w.cy0 - w.y0):S * (w.cy1 - w.y0), S * (w.cx0 - w.x0):S * (w.cx1 - w.x0)]
    return out
