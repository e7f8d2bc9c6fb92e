"""Weight tables of the target resampler (hrn_resample_targets, include/hrnet_hip.h): HR / SM stored at `R * side` resampled to
`scale * side` when a DeviceImagesetCache is built with resample_targets=True.  Host only, numpy, fp64: the kernel multiplies
and adds what is computed here, so the device and a reference share their weights and differ in summation order alone.

Per axis: n_in = R * side, n_out = scale * side, f = max(1, R / scale).  Output sample j sits at source coordinate
x_j = (j + 0.5) * R / scale - 0.5; its weight on source sample k is L3((k - x_j) / f), L3(t) = sinc(t) sinc(t / 3) for |t| < 3,
else 0 (a Lanczos-3 window, widened by f when shrinking so that it also low-passes).  Taps outside 0 .. n_in - 1 are dropped and
the remaining weights divided by their sum.  The 2-D filter is the separable product of the two axes."""
import numpy as np

MAX_TAPS = 12           # HRN_RESAMPLE_TAPS: 6 f taps at most, f <= 2
SCALES = (2, 3, 4)


def check_scale(scale, what="scale"):
    if isinstance(scale, bool) or not isinstance(scale, (int, np.integer)) or int(scale) not in SCALES:
        raise ValueError(f"{what} must be 2, 3 or 4, got {scale!r}")
    return int(scale)


def weight_table(side, R, scale):
    """-> (first (n_out,) int32, count (n_out,) int32, weights (n_out, MAX_TAPS) float64, zero beyond count): output sample j
    reads source samples first[j] .. first[j] + count[j] - 1."""
    R, scale = check_scale(R, "stored ratio"), check_scale(scale)
    if side <= 0:
        raise ValueError(f"side must be positive, got {side}")
    n_in, n_out = R * side, scale * side
    f = max(1.0, R / scale)
    first = np.zeros(n_out, np.int32)
    count = np.zeros(n_out, np.int32)
    weights = np.zeros((n_out, MAX_TAPS), np.float64)
    for j in range(n_out):
        x = (j + 0.5) * R / scale - 0.5
        k = np.arange(max(0, int(np.floor(x - 3.0 * f)) - 1), min(n_in - 1, int(np.ceil(x + 3.0 * f)) + 1) + 1)
        t = (k - x) / f
        keep = np.abs(t) < 3.0
        k, t = k[keep], t[keep]
        w = np.sinc(t) * np.sinc(t / 3.0)
        w = w / np.sum(w)
        if not 0 < len(k) <= MAX_TAPS:
            raise AssertionError(f"{len(k)} taps for output {j} of ({side}, {R}, {scale})")
        first[j], count[j] = k[0], len(k)
        weights[j, :len(k)] = w
    return first, count, weights
