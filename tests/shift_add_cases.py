"""The cases of the shift-and-add tests (tests/test_shift_add_host.py on the CPU, tests/test_gpu_shift_add.py on the device), made once:
six shapes x three scales x the seven kinds of shifts, and over them - by a fixed mixing of the case's index, so that every value meets
every scale and every kind of shift - the three sigmas, the two priors, the four kinds of masks and the three kinds of alphas.  The
restatement's results are cached with the case: a reference is computed once and shared."""
import functools

import numpy as np

import shift_add_ref as R

TH, TW = 8, 32                                       # binding.SHIFT_ADD_TILE (tests/test_shift_add_host.py checks the two agree)
SHAPES = [(2, 1, 1, 1), (1, 3, 2, 5), (2, 4, 5, 7), (1, 9, 2 * TH - 1, 2 * TW + 1), (2, 5, 2 * TH + 1, 2 * TW - 1), (1, 33, TH, TW)]
SCALES = [2, 3, 4]
SIGMAS = [0.1, 0.25, 1.0]
PRIORS = [0.0, 0.05]
SHIFTS = ["zeros", "whole", "halves", "whole-eps", "random", "far", "nan"]
MASKS = ["none", "random", "one-view", "block"]
ALPHAS = ["none", "some-zero", "sample-zero"]
EPS = 1e-7


def plan():
    """-> [(shape, scale, shifts, sigma, prior, masks, alphas)], 126 cases"""
    out = []
    for si, shape in enumerate(SHAPES):
        for ci, scale in enumerate(SCALES):
            for k, kind in enumerate(SHIFTS):
                sigma, prior = SIGMAS[(k + ci + si) % 3], PRIORS[(k + si) % 2]
                if (kind, scale, sigma) == ("halves", 4, 0.1):
                    # every sample of every view then lies 0.125 or 0.375 or more from an HR pixel, and k(0.375)^2 = 7.7e-7 is the
                    # fallback's threshold itself: with prior 0 a quarter of the pixels would sit on it
                    prior = PRIORS[1]
                out.append((shape, scale, kind, sigma, prior, MASKS[(k + 2 * ci + si) % 4], ALPHAS[(k + ci + 2 * si) % 3]))
    return out


def case_id(c):
    shape, scale, kind, sigma, prior, masks, alphas = c
    return f"{'x'.join(map(str, shape))}-x{scale}-{kind}-s{sigma}-p{prior}-{masks}-{alphas}"


def block_of(H, W):
    """the block the `block` masks hide in every view: the middle half of each axis (at least one pixel)"""
    return slice(H // 4, max(H - H // 4, H // 4 + 1)), slice(W // 4, max(W - W // 4, W // 4 + 1))


MAX_EXCLUDED = 1e-3                                  # the largest share of a case's pixels at the fallback's threshold


@functools.lru_cache(maxsize=None)
def inputs(c):
    """-> dict of numpy f32 inputs: views, masks (or None), alphas (or None), shifts, base, g (an output gradient).  The pixels whose
    D + prior lies within a factor of two of the fallback's threshold are left out of a comparison with the device; a case is drawn
    again (the next salt of its seed) until the restatement alone has at most MAX_EXCLUDED of its pixels there."""
    shape, scale, kind, sigma, prior, mkind, akind = c
    for salt in range(64):
        x = _draw(c, salt)
        D = R.sums(x["views"], x["masks"], x["alphas"], x["shifts"], scale, sigma)[1]
        if float(R.excluded(D + float(np.float32(prior))).mean()) <= MAX_EXCLUDED:
            return x
    raise AssertionError(f"{case_id(c)}: no draw with at most {MAX_EXCLUDED} of its pixels at the threshold")


def _draw(c, salt):
    shape, scale, kind, sigma, prior, mkind, akind = c
    B, V, H, W = shape
    rng = np.random.Generator(np.random.PCG64(1000 * sum((k + 1) * ord(ch) for k, ch in enumerate(case_id(c))) + salt))
    views = rng.uniform(0.05, 1.0, shape).astype(np.float32)
    rand = rng.uniform(-3.5, 3.5, (B, V, 2)).astype(np.float32)
    if kind == "zeros":
        shifts = np.zeros((B, V, 2), np.float32)
    elif kind == "whole":
        shifts = rng.choice(np.array([-2, -1, 1, 2], np.float32), (B, V, 2))
    elif kind == "halves":
        shifts = rng.choice(np.array([-2.5, -1.5, -0.5, 0.5, 1.5, 2.5], np.float32), (B, V, 2))
    elif kind == "whole-eps":
        shifts = (rng.choice(np.array([-2, -1, 0, 1, 2], np.float64), (B, V, 2)) + rng.choice(np.array([-EPS, EPS]), (B, V, 2))).astype(np.float32)
    else:
        shifts = rand
        if kind == "far":
            shifts[:, V // 2] = (300.0, -300.0)
        if kind == "nan":
            shifts[:, V // 2, 1] = np.nan
    masks = None
    if mkind == "random":
        masks = (rng.uniform(0, 1, shape) >= 0.3).astype(np.float32)
    elif mkind == "one-view":
        masks = np.ones(shape, np.float32)
        masks[:, V - 1] = 0
    elif mkind == "block":
        masks = (rng.uniform(0, 1, shape) >= 0.1).astype(np.float32) * rng.choice(np.array([1.0, 2.0, -1.0], np.float32), shape)
        ys, xs = block_of(H, W)
        masks[:, :, ys, xs] = 0
    alphas = None
    if akind == "some-zero":
        alphas = (rng.uniform(0, 1, (B, V)) >= 0.4).astype(np.float32) * rng.choice(np.array([1.0, 0.5], np.float32), (B, V))
        alphas[:, 0] = 1
    elif akind == "sample-zero":
        alphas = np.ones((B, V), np.float32)
        alphas[B - 1] = 0
    base = rng.uniform(-1, 1, (B, scale * H, scale * W)).astype(np.float32)
    g = rng.uniform(-1, 1, (B, scale * H, scale * W)).astype(np.float32)
    return dict(views=views, masks=masks, alphas=alphas, shifts=shifts, base=base, g=g)


@functools.lru_cache(maxsize=None)
def reference(c, with_base=True):
    """-> dict: out, D, T, den, keep (the pixels compared) of the restatement; with_base False: base NULL (its prior must be 0)"""
    shape, scale, kind, sigma, prior, mkind, akind = c
    x = inputs(c)
    out, D, T, den = R.forward(x["views"], x["masks"], x["alphas"], x["shifts"], scale, sigma, prior, x["base"] if with_base else None)
    return dict(out=out, D=D, T=T, den=den, keep=~R.excluded(den))


@functools.lru_cache(maxsize=None)
def reference_adjoint(c):
    """the adjoint at g with weight = the restatement's D rounded to fp32 -> dict: weight (f32), d_views, T_views, d_base, T_base"""
    shape, scale, kind, sigma, prior, mkind, akind = c
    B, V, H, W = shape
    x = inputs(c)
    weight = reference(c)["D"].astype(np.float32)
    dv, Tv, db, Tb = R.adjoint(x["g"], weight, x["masks"], x["alphas"], x["shifts"], V, H, W, scale, sigma, prior)
    return dict(weight=weight, d_views=dv, T_views=Tv, d_base=db, T_base=Tb)
