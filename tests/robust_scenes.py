"""The three scenes of the robust-reconstruction quality table (tests/test_robust_host.py on the restatement,
tests/test_gpu_robust_quality.py on the device): tests/shift_add_scene.py's scene of 48 x 48 views at x3, nine views shifted by up to
1.5 px, two cloud discs per view, with the noise and the number of views whose clouds the masks do NOT show varied; true shifts; the start
is shift-and-add with sigma 0.25 and no prior; scored by the interior PSNR, 12 HR pixels off every side.  Results of the restatement are
cached: a reference is computed once and shared."""
import functools

import numpy as np

import robust_ref as RB
import shift_add_ref as R
import shift_add_scene as SS

SCALE, SIGMA, BORDER, STEP = 3, 0.25, 12, 1.0
SCENES = [(0.02, 0), (0.005, 2), (0.02, 2)]                 # (noise, views with unmasked clouds)
DELTA, LAM, P, ALPHA, EPS = 0.1, 4e-4, 2, 0.7, 0.02        # the defaults of hrnet_hip.observation.reconstruct
METHODS = {"plain": dict(robust=False, lam=0.0), "welsch": dict(robust=True, lam=0.0), "btv": dict(robust=False, lam=LAM),
           "welsch+btv": dict(robust=True, lam=LAM)}
# the three orderings the table is built for: (scene, method, iterations, margin in dB over plain back-projection)
ORDERINGS = [((0.005, 2), "welsch", 10, 1.0), ((0.02, 0), "btv", 30, 1.0), ((0.02, 2), "welsch+btv", 30, 1.0)]


@functools.lru_cache(maxsize=None)
def scene(noise, unmasked):
    sc = SS.make(n_lr=48, scale=SCALE, views=9, band=0.25, limit=1.5, noise=noise, clouds=2, margin=3.0, seed=1)
    for v in range(1, 1 + unmasked):
        sc["masks"][0, v] = 1
    sc["start"] = R.forward(sc["lrs"], sc["masks"], None, sc["shifts"], SCALE, SIGMA, 0.0)[0].astype(np.float32)
    return sc


def psnr(x, sc):
    return SS.psnr(np.asarray(x, np.float64)[0], sc["hr"], BORDER)


@functools.lru_cache(maxsize=None)
def restated(noise, unmasked, method, iters, delta=DELTA, lam=None):
    """-> (the restatement's frame after `iters` iterations from the scene's start, its PSNR)"""
    sc = scene(noise, unmasked)
    kw = dict(METHODS[method], delta=delta)
    if lam is not None:
        kw["lam"] = lam
    x, _, _ = RB.reconstruct(sc["start"], sc["lrs"], sc["masks"], None, sc["shifts"], SCALE, iters, STEP, True, P=P, alpha=ALPHA, eps=EPS, **kw)
    return x, psnr(x, sc)
