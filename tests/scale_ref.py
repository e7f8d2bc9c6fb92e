"""Helpers of the x2 / x4 input-pipeline tests (test_scale_pipeline_host.py, test_gpu_scale_pipeline.py): synthetic imagesets
whose HR / SM files are stored at any HR / LR ratio, a numpy restatement of the loader at a target scale, and the fp64 numpy
reference of the target resampler, written from its definition:

    per axis  n_in = R side, n_out = scale side, f = max(1, R / scale), x_j = (j + 0.5) R / scale - 0.5,
    weight of source sample k on output j: L3((k - x_j) / f), L3(t) = sinc(t) sinc(t / 3) for |t| < 3 else 0, taps outside
    0 .. n_in - 1 dropped, the rest divided by their sum;  HR = clip(A U A^T, 0, 65535) rounded half to even;
    SM clear iff every source sample under a non-zero weight (both axes) is clear.
"""
import os

import numpy as np

from imageset_png import write_png

PAIRS = [(2, 3), (2, 4), (3, 2), (3, 4), (4, 2), (4, 3)]


def write_scaled_imageset(root, name, n_views, ratio, lr=128, with_hr=True, seed=0, lr_views=None, hr=None, sm=None):
    """imageset_png.write_imageset with HR / SM stored at `ratio` times the LR side (that one is x3 only)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    d = os.path.join(root, name)
    os.makedirs(d)
    n = ratio * lr
    np.save(os.path.join(d, "clearance.npy"), rng.random(n_views))            # first, then the LR views: the same at every ratio
    for v in range(n_views):
        a = lr_views[v] if lr_views is not None else rng.integers(0, 16000, (lr, lr), dtype=np.uint16)
        if lr_views is None:
            a[3:9, 5:40] = 65535
        write_png(os.path.join(d, f"LR{v:03d}.png"), a)
        write_png(os.path.join(d, f"QM{v:03d}.png"), (rng.random((lr, lr)) > 0.2).astype(np.uint8) * 255)
    if sm is None:
        sm = (rng.random((n, n)) > 0.1) * rng.integers(1, 256, (n, n))           # any non-zero sample counts as clear
    write_png(os.path.join(d, "SM.png"), np.asarray(sm).astype(np.uint8))
    if with_hr:
        write_png(os.path.join(d, "HR.png"), hr if hr is not None else rng.integers(0, 65536, (n, n), dtype=np.uint16))
    return d


def restated_read(d, create_patches, patch_size, seed, top_k, beta, scale, decode):
    """read_imageset + the float conversion of __getitem__ at `scale`, restated on numpy; `decode(path)` -> uint16 (H, W).
    Makes the loader's numpy RNG calls (one choice, then two randint, each after an optional re-seed)."""
    names = np.sort(np.array([f[2:-4] for f in os.listdir(d) if f.startswith("QM") and f.endswith(".png")]))
    cl = np.load(os.path.join(d, "clearance.npy"))
    if top_k is not None and top_k > 0:
        if seed is not None:
            np.random.seed(seed)
        e = np.exp(beta * cl / cl.max())
        i = np.random.choice(range(len(e)), size=min(top_k, len(names)), p=e / e.sum(), replace=False)
        names, cl = names[i], cl[i]
    else:
        o = np.argsort(cl)[::-1]
        names, cl = names[o], cl[o]
    lr = np.array([decode(os.path.join(d, f"LR{i}.png")) for i in names], dtype=np.uint16)
    sm = decode(os.path.join(d, "SM.png")) != 0
    hr = decode(os.path.join(d, "HR.png")).astype(np.uint16) if os.path.exists(os.path.join(d, "HR.png")) else None
    x = y = 0
    if create_patches:
        if seed is not None:
            np.random.seed(seed)
        x = np.random.randint(low=0, high=lr.shape[1] - patch_size)
        y = np.random.randint(low=0, high=lr.shape[2] - patch_size)
        k, P = scale, patch_size
        lr = lr[:, x:x + P, y:y + P]
        sm = sm[k * x:k * x + k * P, k * y:k * y + k * P]
        if hr is not None:
            hr = hr[k * x:k * x + k * P, k * y:k * y + k * P]
    f = lambda a: (a / 65535.0).astype(np.float32)
    return dict(names=names, corner=(x, y), lr_u16=lr, lr=f(lr), hr_u16=hr, hr=None if hr is None else f(hr), sm=sm, cl=cl)


def restated_batch(dirs, min_L, create_patches, patch_size, seed, top_k, beta, scale, decode):
    """load_batch restated: (lrs, alphas, hrs or [], maps, names) as numpy float32, views truncated / zero-padded to min_L."""
    items = [restated_read(d, create_patches, patch_size, seed, top_k, beta, scale, decode) for d in dirs]
    S = items[0]["lr"].shape[-1]
    lrs = np.zeros((len(items), min_L, S, S), np.float32)
    alphas = np.zeros((len(items), min_L), np.float32)
    for b, it in enumerate(items):
        n = min(min_L, len(it["lr"]))
        lrs[b, :n], alphas[b, :n] = it["lr"][:n], 1
    have_hr = all(it["hr"] is not None for it in items)
    hrs = np.stack([it["hr"] for it in items]) if have_hr else []
    return lrs, alphas, hrs, np.stack([it["sm"].astype(np.float32) for it in items]), [os.path.basename(d) for d in dirs]


# ------------------------------------------------------------------ the resampler's reference
def ref_matrix(side, R, scale):
    """Dense (n_out, n_in) fp64 matrix of one axis, straight from the definition."""
    n_in, n_out = R * side, scale * side
    f = max(1.0, R / scale)
    A = np.zeros((n_out, n_in), np.float64)
    k = np.arange(n_in)
    for j in range(n_out):
        x = (j + 0.5) * R / scale - 0.5
        t = (k - x) / f
        taps = np.flatnonzero(np.abs(t) < 3.0)
        w = np.sinc(t[taps]) * np.sinc(t[taps] / 3.0)
        A[j, taps] = w / np.sum(w)
    return A


def ref_resample_hr(u, side, R, scale):
    """-> (uint16 result, unrounded fp64 values before the clip)"""
    A = ref_matrix(side, R, scale)
    v = A @ u.astype(np.float64) @ A.T
    return np.rint(np.clip(v, 0.0, 65535.0)).astype(np.uint16), v


def ref_resample_sm(clear, side, R, scale):
    """clear: bool (n_in, n_in) -> bool (n_out, n_out)"""
    N = (ref_matrix(side, R, scale) != 0).astype(np.float64)
    return (N @ (~clear).astype(np.float64) @ N.T) == 0          # counts of unclear samples under the filter: exact in fp64


def near_half(v, eps=1e-6):
    """Samples whose unrounded value (after the clip) is within eps of a half-integer: either neighbour is a fair rounding."""
    c = np.clip(v, 0.0, 65535.0)
    return np.abs(c - np.floor(c) - 0.5) <= eps


def field_image(side_px, seed, noise=1500.0):
    """uint16 test image: a smooth field plus noise, with a saturated block and a zero block, so that the resampler's ringing
    is clipped at both ends."""
    g = np.random.Generator(np.random.PCG64(seed))
    y, x = np.mgrid[0:side_px, 0:side_px] / side_px
    v = 30000 + 20000 * np.sin(2 * np.pi * (1.5 * x + 0.3 * g.random())) * np.cos(2 * np.pi * (1.1 * y + 0.2)) + noise * g.standard_normal((side_px, side_px))
    a = np.clip(np.rint(v), 0, 65535).astype(np.uint16)
    q = side_px // 8
    a[q:3 * q, 2 * q:4 * q] = 65535
    a[5 * q:7 * q, q:3 * q] = 0
    return a


def blob_mask(side_px, seed):
    """bool clear-mask with blob-shaped unclear regions: a disc, a bar, an edge strip and one isolated pixel."""
    g = np.random.Generator(np.random.PCG64(seed))
    y, x = np.mgrid[0:side_px, 0:side_px]
    n = side_px
    cy, cx = (0.3 + 0.4 * g.random(2)) * n
    clear = (y - cy) ** 2 + (x - cx) ** 2 > (0.08 * n) ** 2
    clear[int(0.8 * n):int(0.8 * n) + max(2, n // 40), n // 10:n // 2] = False
    clear[:, :max(1, n // 60)] = False
    clear[int(0.15 * n), int(0.85 * n)] = False
    return clear
