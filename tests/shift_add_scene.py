"""The synthetic scene of tests/test_gpu_shift_add_quality.py: a periodic, band-limited HR image, its LR views - translated by known
sub-pixel shifts with a Fourier phase ramp, averaged over S x S boxes, decimated, with cloud discs in the masks and a little noise - and
the interior PSNR the predictors are scored with."""
import numpy as np


def make(n_lr=40, scale=3, views=9, band=0.3, limit=1.5, noise=0.005, clouds=2, margin=3.0, seed=0):
    """-> dict: hr (S n, S n) fp64 in about [0, 1]; lrs (1, V, n, n) f32; masks (1, V, n, n) f32 (1 clear, 0 cloud); shifts (1, V, 2) f32,
    view 0 at (0, 0), in the registration convention Registered(y, x) = View(y + dy, x + dx).  band: the HR image's band limit in cycles
    per HR pixel (the LR Nyquist is 0.5 / S: above it the views alias); a 1 / f amplitude spectrum."""
    rng = np.random.Generator(np.random.PCG64(seed))
    N = n_lr * scale
    fy, fx = np.meshgrid(np.fft.fftfreq(N), np.fft.fftfreq(N), indexing="ij")
    f = np.hypot(fy, fx)
    amp = np.where((f > 0) & (f <= band), 1.0 / np.maximum(f, 1.0 / N), 0.0)
    spec = amp * np.exp(2j * np.pi * rng.uniform(0, 1, (N, N)))
    z = np.real(np.fft.ifft2(spec))
    hr = 0.5 + 0.18 * z / z.std()
    shifts = rng.uniform(-limit, limit, (views, 2))
    shifts[0] = 0.0
    shifts = shifts.astype(np.float32)
    F = np.fft.fft2(hr)
    lrs = np.zeros((views, n_lr, n_lr), np.float32)
    masks = np.ones((views, n_lr, n_lr), np.float32)
    yy, xx = np.meshgrid(np.arange(n_lr), np.arange(n_lr), indexing="ij")
    for v in range(views):
        # View(y') = Scene(y' - dy): the scene translated by +dy LR pixels = S dy HR pixels
        ramp = np.exp(-2j * np.pi * (fy * scale * float(shifts[v, 0]) + fx * scale * float(shifts[v, 1])))
        moved = np.real(np.fft.ifft2(F * ramp))
        lr = moved.reshape(n_lr, scale, n_lr, scale).mean((1, 3))
        lrs[v] = (lr + noise * rng.standard_normal(lr.shape)).astype(np.float32)
        for _ in range(clouds if v else 0):               # the reference view stays clear
            cy, cx, r = rng.uniform(0, n_lr), rng.uniform(0, n_lr), rng.uniform(2.0, 5.0)
            d2 = (yy - cy) ** 2 + (xx - cx) ** 2
            lrs[v][d2 <= r * r] = 0.95                      # a cloud is bright,
            masks[v][d2 <= (r + margin) ** 2] = 0           # and its mask is drawn with a margin, as quality masks are
    return dict(hr=hr, lrs=lrs[None], masks=masks[None], shifts=shifts[None])


def psnr(sr, hr, border):
    """the PSNR of sr against hr (peak 1) over the interior: `border` HR pixels left off every side"""
    d = (np.asarray(sr, np.float64) - hr)[border:-border, border:-border]
    return float(-10.0 * np.log10(np.mean(d * d)))
