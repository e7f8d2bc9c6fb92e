"""The shift-searched, brightness-corrected SSIM (cSSIM; include/hrnet_hip.h) restated in fp64 numpy, in the DIRECT
form: X = m g, Y = m (s + bias), and X, Y, X^2, Y^2, XY are filtered per offset - no bias algebra, no field shared between offsets.  The
kernel (csrc/cssim.hip) centres its fields per tile and shares three of them between the offsets; this does neither, so the two share
only the definition.  Also the test scenes, a float32 model of the kernel's algebra, and wrong variants of the restatement as controls."""
import numpy as np

TAPS = {"gaussian": 11, "uniform": 7}


def window(name):
    """-> (taps (T,) fp64, cov_norm).  The Gaussian's taps are the fp32 values the definition states, held in fp64."""
    if name == "gaussian":
        x = np.arange(-5, 6, dtype=np.float64)
        g = np.exp(-x * x / (2.0 * 1.5 ** 2))
        return (g / g.sum()).astype(np.float32).astype(np.float64), 1.0
    if name == "uniform":
        return np.full(7, 1.0 / 7.0), 49.0 / 48.0
    raise ValueError(name)


def filter_valid(a, taps):
    """The separable window over the positions where it fits: (h, w) -> (h - T + 1, w - T + 1)."""
    T = len(taps)
    h, w = a.shape
    rows = sum(taps[o] * a[o:o + h - T + 1] for o in range(T))
    return sum(taps[o] * rows[:, o:o + w - T + 1] for o in range(T))


def ssim_map(X, Y, taps, cov_norm, data_range):
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mx, my = filter_valid(X, taps), filter_valid(Y, taps)
    vx = cov_norm * (filter_valid(X * X, taps) - mx * mx)
    vy = cov_norm * (filter_valid(Y * Y, taps) - my * my)
    vxy = cov_norm * (filter_valid(X * Y, taps) - mx * my)
    return ((2 * mx * my + c1) * (2 * vxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))


def shift_cssim(sr, hr, hr_map, border=3, window_name="gaussian", clip=True, correct_bias=True, data_range=1.0):
    """One sample, (H, W) arrays -> (scores (nk,) fp64 with -inf where n_k = 0, k* (-1 without an eligible offset), bias (nk,), n (nk,))."""
    sr, hr = np.asarray(sr, np.float64), np.asarray(hr, np.float64)
    m_full = (np.asarray(hr_map) != 0).astype(np.float64)
    taps, cov_norm = window(window_name)
    H, W = sr.shape
    h, w = H - 2 * border, W - 2 * border
    s = sr[border:border + h, border:border + w]
    if clip:
        s = np.where(np.isnan(s), s, np.clip(s, 0.0, 1.0))
    nb = 2 * border + 1
    scores, bias, cnt = np.full(nb * nb, -np.inf), np.zeros(nb * nb), np.zeros(nb * nb)
    with np.errstate(invalid="ignore", divide="ignore"):
        for u in range(nb):
            for v in range(nb):
                k = u * nb + v
                g, m = hr[u:u + h, v:v + w], m_full[u:u + h, v:v + w]
                cnt[k] = m.sum()
                if cnt[k] == 0:
                    continue
                bias[k] = (m * (g - s)).sum() / cnt[k] if correct_bias else 0.0
                scores[k] = ssim_map(m * g, m * (s + bias[k]), taps, cov_norm, data_range).mean()
    best, bv = -1, -np.inf
    for k in range(nb * nb):
        if cnt[k] > 0 and scores[k] > bv:
            best, bv = k, scores[k]
    return scores, best, bias, cnt


def smooth_field(rng, H, W, passes=3):
    """A smoothed random field in about [0.1, 0.9]: structure at the scale of the windows."""
    a = rng.random((H + 8, W + 8))
    for _ in range(passes):
        a = (a + np.roll(a, 1, 0) + np.roll(a, -1, 0) + np.roll(a, 1, 1) + np.roll(a, -1, 1)) / 5.0
    a = a[4:-4, 4:-4]
    a = (a - a.min()) / (a.max() - a.min())
    return 0.1 + 0.8 * a


def scene(seed, H, W, shift=(1, -2)):
    """-> (sr, hr, map) float32: hr a smoothed field, sr = hr displaced by `shift` (sr[y, x] = hr[y + dy, x + dx], so the search finds
    the offset (border + dy, border + dx)), x 0.9 + 0.03 plus noise of sigma 0.02, the map with 15 % holes and a rectangular blob."""
    rng = np.random.default_rng(seed)
    big = smooth_field(rng, H + 16, W + 16)
    hr = big[8:8 + H, 8:8 + W]
    sr = big[8 + shift[0]:8 + shift[0] + H, 8 + shift[1]:8 + shift[1] + W] * 0.9 + 0.03 + rng.normal(0.0, 0.02, (H, W))
    m = (rng.random((H, W)) > 0.15).astype(np.float32)
    m[H // 3:H // 3 + max(2, H // 5), W // 4:W // 4 + max(2, W // 4)] = 0.0
    return sr.astype(np.float32), hr.astype(np.float32), m


def gap(scores):
    """best - runner-up among the finite scores."""
    f = np.sort(scores[np.isfinite(scores)])
    return f[-1] - f[-2] if len(f) > 1 else np.inf


# ----------------------------------------------------------------------------- the pinning pass (tests/test_cssim_pin_host.py,
# tests/test_gpu_cssim_pin.py): clear low-contrast scenes, a float32 model of the kernel's algebra, and wrong variants as controls
MASKS = ("clear", "blob", "edge")


def scene_clear(seed, H, W, level=0.9, contrast=0.05, mask="clear", shift=(1, -2)):
    """-> (sr, hr, map) float32: a bright (or dark), low-contrast, mostly clear frame - snow, haze - which `scene`'s 15 % holes never give:
    hr = level + contrast (field - 0.5); sr the same field displaced by `shift`, with gain 0.9 about `level`, plus noise of sigma
    0.4 contrast.  mask: "clear" all ones; "blob" one rectangle of 5 x 6 zeros; "edge" the left third masked, so that a tile holds fully
    masked, fully clear and mixed windows at once."""
    rng = np.random.default_rng(seed)
    big = smooth_field(rng, H + 16, W + 16)
    hr = level + contrast * (big[8:8 + H, 8:8 + W] - 0.5)
    moved = big[8 + shift[0]:8 + shift[0] + H, 8 + shift[1]:8 + shift[1] + W]
    sr = level + 0.9 * contrast * (moved - 0.5) + rng.normal(0.0, 0.4 * contrast, (H, W))
    m = np.ones((H, W), np.float32)
    if mask == "blob":
        m[H // 3:H // 3 + 5, W // 3:W // 3 + 6] = 0.0
    elif mask == "edge":
        m[:, :W // 3] = 0.0
    elif mask != "clear":
        raise ValueError(mask)
    return sr.astype(np.float32), hr.astype(np.float32), m


def _filter32(a, taps):
    """filter_valid in float32: every product and every sum rounded, the taps in index order, down the columns first as the kernel does"""
    T = len(taps)
    h, w = a.shape
    rows = taps[0] * a[0:h - T + 1]
    for o in range(1, T):
        rows = rows + taps[o] * a[o:o + h - T + 1]
    out = taps[0] * rows[:, 0:w - T + 1]
    for o in range(1, T):
        out = out + taps[o] * rows[:, o:o + w - T + 1]
    assert out.dtype == np.float32
    return out


MODEL_TH, MODEL_WIN = 16, 64         # csrc/cssim.hip: CS_TH, CS_WIN (tests/test_gpu_cssim.py asserts them against the source)


def shift_cssim_f32(sr, hr, hr_map, border=3, window_name="gaussian", clip=True, correct_bias=True, data_range=1.0, form="centred"):
    """A MODEL of csrc/cssim.hip's arithmetic in float32 numpy, NOT a reference: it shares the kernel's decomposition (six filtered
    fields, three of the hr position and three per offset), its tiles, its fp32 SSIM and its fp64 means, so that the conditioning of
    that algebra shows on a machine without a GPU.  It is not the kernel either: numpy fuses no multiply-add and sums in another order.
    -> scores (nk,) fp64, as `shift_cssim`'s first result.

    form="uncentred": the kernel as it first shipped.  X = m g, Y = m (s + b); G m, G(m g), G(m g^2) and G(m s), G(m s^2), G(m g s) are
    filtered, the bias b enters by algebra, and v = cov_norm (G X^2 - mu^2) is the difference of two numbers of the size of level^2.
    form="centred": the kernel now.  Per tile, c is the mean of g over the clear pixels of the staged hr window;
    X~ = m (g - c), Y~ = m (s + b - c), w = G(1 - m) - (S - 1) with S the squared sum of the definition's taps (so G m = 1 - w exactly);
        mu_x = G X~ + c (1 - w)                         v_x / cov_norm = (G X~^2 - (G X~)^2) + 2 c w G X~ + c^2 w (1 - w)
        v_xy / cov_norm = (G X~Y~ - G X~ G Y~) + c w (G X~ + G Y~) + c^2 w (1 - w),   mu_y, v_y as mu_x, v_x.
    In a clear window w = -(S - 1) and what is subtracted has the size of the contrast, not of the level."""
    f32 = np.float32
    sr, hr = np.asarray(sr, f32), np.asarray(hr, f32)
    m_full = (np.asarray(hr_map) != 0).astype(f32)
    taps64, cov_norm = window(window_name)
    taps, cn = taps64.astype(f32), f32(cov_norm)
    delta = f32(taps64.sum() ** 2 - 1.0)            # the definition's taps: 0 for the uniform window (7 x 1/7 in fp64, to 1e-16)
    T = len(taps)
    H, W = sr.shape
    h, w = H - 2 * border, W - 2 * border
    mh, mw = h - T + 1, w - T + 1
    s_all = sr[border:border + h, border:border + w]
    if clip:
        s_all = np.where(np.isnan(s_all), s_all, np.clip(s_all, f32(0), f32(1))).astype(f32)
    nb = 2 * border + 1
    c1, c2 = f32(f32(0.01) * f32(data_range)) ** 2, f32(f32(0.03) * f32(data_range)) ** 2
    TW = MODEL_WIN - T + 1
    scores = np.full(nb * nb, -np.inf)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in range(nb * nb):
            u, v = divmod(k, nb)
            g_k, m_k = hr[u:u + h, v:v + w], m_full[u:u + h, v:v + w]
            n = float(m_k.sum(dtype=np.float64))
            if n == 0:
                continue
            b64 = float((m_k.astype(np.float64) * (g_k.astype(np.float64) - s_all)).sum() / n) if correct_bias else 0.0
            total = 0.0
            for y0 in range(0, mh, MODEL_TH):
                for x0 in range(0, mw, TW):
                    rows, cols = slice(y0, min(h, y0 + MODEL_TH + T - 1)), slice(x0, min(w, x0 + MODEL_WIN))
                    s, g, m = s_all[rows, cols], g_k[rows, cols], m_k[rows, cols]
                    if form == "uncentred":
                        b = f32(b64)
                        gm, gmg, gmgg = _filter32(m, taps), _filter32(m * g, taps), _filter32(m * g * g, taps)
                        ms, mss, mgs = _filter32(m * s, taps), _filter32(m * s * s, taps), _filter32(m * g * s, taps)
                        mux, muy = gmg, b * gm + ms
                        eyy = (b * b) * gm + ((f32(2) * b) * ms + mss)
                        exy = b * gmg + mgs
                        vx, vy, vxy = cn * (gmgg - mux * mux), cn * (eyy - muy * muy), cn * (exy - mux * muy)
                    elif form == "centred":
                        win_g = hr[y0:min(H, y0 + MODEL_TH + T - 1 + 2 * border), x0:min(W, x0 + MODEL_WIN + 2 * border)]
                        win_m = m_full[y0:min(H, y0 + MODEL_TH + T - 1 + 2 * border), x0:min(W, x0 + MODEL_WIN + 2 * border)]
                        cnt = win_m.sum(dtype=np.float64)
                        c = f32((win_m * win_g).sum(dtype=np.float64) / cnt) if cnt > 0 else f32(0)
                        c = c if np.isfinite(c) else f32(0)
                        x, t = m * (g - c), s - f32(np.float64(c) - b64)
                        mt = m * t
                        ww = _filter32(f32(1) - m, taps) - delta
                        ax, axx = _filter32(x, taps), _filter32(x * x, taps)
                        ay, ayy, axy = _filter32(mt, taps), _filter32(mt * t, taps), _filter32(x * t, taps)
                        cp, cw = c * (f32(1) - ww), c * ww
                        e = cp * cw
                        mux, muy = ax + cp, ay + cp
                        vx = cn * (((axx - ax * ax) + (f32(2) * cw) * ax) + e)
                        vy = cn * (((ayy - ay * ay) + (f32(2) * cw) * ay) + e)
                        vxy = cn * (((axy - ax * ay) + cw * (ax + ay)) + e)
                    else:
                        raise ValueError(form)
                    ssim = ((f32(2) * mux * muy + c1) * (f32(2) * vxy + c2)) / ((mux * mux + muy * muy + c1) * (vx + vy + c2))
                    assert ssim.dtype == np.float32
                    total += ssim[:min(MODEL_TH, mh - y0), :min(TW, mw - x0)].sum(dtype=np.float64)
            scores[k] = total / (mh * mw)
    return scores


CONTROLS = ("tap_dropped", "neighbouring_offset", "cov_norm_one", "bias_left_out", "map_as_weight", "pixel_left_out", "row_left_out")


def shift_cssim_control(name, sr, hr, hr_map, border=3, window_name="gaussian", clip=True, correct_bias=True, data_range=1.0):
    """`shift_cssim`'s scores with one thing wrong - what a kernel that made this mistake would return:
    tap_dropped          the window's last tap is 0
    neighbouring_offset  hr and map are cropped at (u, v + 1) (at (u, v - 1) in the last column of offsets)
    cov_norm_one         cov_norm = 1 (differs under the uniform window only)
    bias_left_out        Y = m s: n_k and the search as they are, the bias not added
    map_as_weight        m = the map's value rather than (map != 0), as the searched loss beside it weights (differs for maps that are not 0 / 1)
    pixel_left_out       the map's last pixel is missing from the sum; the divisor is the whole map's size, as a wrong `valid` bit would leave it
    row_left_out         the map's last row is missing from the sum, the divisor unchanged: a tile remainder not walked"""
    assert name in CONTROLS, name
    sr, hr = np.asarray(sr, np.float64), np.asarray(hr, np.float64)
    m_full = np.asarray(hr_map, np.float64) if name == "map_as_weight" else (np.asarray(hr_map) != 0).astype(np.float64)
    taps, cov_norm = window(window_name)
    if name == "tap_dropped":
        taps = taps.copy()
        taps[-1] = 0.0
    if name == "cov_norm_one":
        cov_norm = 1.0
    H, W = sr.shape
    h, w = H - 2 * border, W - 2 * border
    s = sr[border:border + h, border:border + w]
    if clip:
        s = np.where(np.isnan(s), s, np.clip(s, 0.0, 1.0))
    nb = 2 * border + 1
    scores = np.full(nb * nb, -np.inf)
    with np.errstate(invalid="ignore", divide="ignore"):
        for u in range(nb):
            for v in range(nb):
                vv = v if name != "neighbouring_offset" else (v + 1 if v + 1 < nb else v - 1)
                g, m = hr[u:u + h, vv:vv + w], m_full[u:u + h, vv:vv + w]
                n = m.sum()
                if n == 0:
                    continue
                bias = (m * (g - s)).sum() / n if correct_bias else 0.0
                ssim = ssim_map(m * g, m * (s + (0.0 if name == "bias_left_out" else bias)), taps, cov_norm, data_range)
                total = ssim.sum()
                if name == "pixel_left_out":
                    total -= ssim[-1, -1]
                if name == "row_left_out":
                    total -= ssim[-1].sum()
                scores[u * nb + v] = total / ssim.size
    return scores
