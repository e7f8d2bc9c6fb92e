"""The shift-searched, brightness-corrected SSIM (cSSIM; include/hrnet_hip.h) restated in fp64 numpy, in the DIRECT
form: X = m g, Y = m (s + bias), and X, Y, X^2, Y^2, XY are filtered per offset - no bias algebra, no field shared between offsets.  The
kernel (csrc/cssim.hip) takes the bias out of the filters; this does not, so the two share only the definition.  Also the test scenes."""
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
