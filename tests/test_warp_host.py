"""CPU: the fp64 restatement of the sampler's backward (tests/warp_ref.py) against itself, and the Python surface of
hrnet_hip.registration.warp where no device is needed.

The restatement: the derivative images of sample_d are the central differences of registration_ref.sample; the derivative taps sum to
zero and are continuous across a whole pixel (the sampler is C^1 there, not C^2: L3'(+-3) = 0 but L3''(+-3) != 0); the gather form of
d_views is the brute-force adjoint, sum g S(e_pq)."""
import os
import sys

import numpy as np
import pytest
import torch

import registration_ref as R
import warp_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = 2.0 ** -10


def _view(H, W, seed):
    return R.scene(H, W, [(0.37, -0.62)], seed)[2][0]


# h = 2^-10: the truncation term h^2 / 6 |S'''| of a central difference is 1.6e-7 |S'''| where S is smooth, and h / 2 times the jump of
# S'' where a whole pixel lies between the two samples; the issue states the tolerances that follow for frames of this kind.
@pytest.mark.parametrize("shift,tol", [((0.25, -1.5), 2e-6), ((-3.75, 4.125), 2e-6), ((2.0, 0.0), 6e-5), ((0.0, 0.0), 6e-5)])
def test_derivative_images_are_the_central_differences(shift, tol):
    T = _view(33, 47, 11)
    S, dy, dx = WR.sample_d(T, shift)
    assert np.array_equal(S, R.sample(T, shift))
    points = [shift, (shift[0] + STEP, shift[1]), (shift[0] - STEP, shift[1]), (shift[0], shift[1] + STEP), (shift[0], shift[1] - STEP)]
    inside = np.logical_and.reduce([R.inside(T.shape, p) for p in points])
    assert inside.sum() > 500
    cy = (R.sample(T, points[1]) - R.sample(T, points[2])) / (2 * STEP)
    cx = (R.sample(T, points[3]) - R.sample(T, points[4])) / (2 * STEP)
    ey, ex = np.abs(cy - dy)[inside].max(), np.abs(cx - dx)[inside].max()
    print(f"shift {shift}: worst |central difference - derivative| dy {ey:.2e} dx {ex:.2e} (images of magnitude {np.abs(dy).max():.2e})")
    assert ey <= tol and ex <= tol
    assert np.abs(dy)[inside].max() > 1e-3 and np.abs(dx)[inside].max() > 1e-3


def test_derivative_taps_sum_to_zero_and_are_continuous_across_a_pixel():
    for f in (0.0, 1e-9, 0.25, 0.5, 0.999, 1.0 - 1e-9):
        assert abs(WR.dtaps(f).sum()) <= 1e-15
    # f -> 1 with n is f = 0 with n + 1: tap o there is tap o + 1 here, and the tap that leaves has L3'(-3) = 0
    left, right = WR.dtaps(1.0 - 1e-9), WR.dtaps(0.0)
    assert np.abs(left[1:] - right[:-1]).max() <= 1e-8 and abs(left[0]) <= 1e-8 and right[-1] == 0.0
    assert np.abs(R.taps(1.0 - 1e-9)[1:] - R.taps(0.0)[:-1]).max() <= 1e-8
    # the series and the closed form of sinc' meet
    for t in (1e-2 * (1 - 1e-12), 1e-2):
        assert abs(float(WR._sinc_slope(t)) - (np.cos(np.pi * t) - np.sinc(t)) / t) <= 1e-13
    # and dtaps is the derivative of taps
    for f in (0.1, 0.37, 0.8):
        assert np.abs((R.taps(f + 1e-6) - R.taps(f - 1e-6)) / 2e-6 - WR.dtaps(f)).max() <= 1e-9


@pytest.mark.parametrize("shift", [(0.37, -0.62), (2.0, 0.0), (-3.75, 4.125), (30.0, 0.0)])
def test_gather_form_is_the_brute_force_adjoint(shift):
    H, W = 19, 23
    rng = np.random.default_rng(5)
    g = rng.standard_normal((H, W))
    valid = rng.random((H, W)) > 0.2
    gm = WR.masked(g, valid, shift)
    brute = np.zeros((H, W))
    for p in range(H):
        for q in range(W):
            e = np.zeros((H, W))
            e[p, q] = 1.0
            brute[p, q] = (gm * R.sample(e, shift)).sum()
    got = WR.d_views(g, valid, shift)
    assert np.abs(got - brute).max() <= 2e-15
    mag, _ = WR.magnitudes(np.ones((H, W)), g, valid, shift)
    assert np.all(got[mag == 0.0] == 0.0) and np.all(np.abs(got) <= mag + 1e-15)
    if shift[0] == 30.0:
        assert not got.any()
    else:
        assert np.abs(got).max() > 0.1
        # the controls of tests/test_gpu_warp.py are mistakes here too
        assert np.abs(WR.d_views(g, valid, shift, reverse=False) - brute).max() > 1e-3
        assert np.abs(WR.d_views(g, valid, shift, whole=0) - brute).max() > 1e-3


def test_d_shifts_is_the_derivative_of_the_weighted_sum():
    T = _view(24, 40, 3)
    rng = np.random.default_rng(9)
    g, valid = rng.standard_normal(T.shape), rng.random(T.shape) > 0.1
    for shift in ((0.25, -1.5), (-3.75, 4.125)):
        def total(s):
            return (WR.masked(g, valid, shift) * R.sample(T, s)).sum()
        want = np.array([(total((shift[0] + STEP, shift[1])) - total((shift[0] - STEP, shift[1]))) / (2 * STEP),
                         (total((shift[0], shift[1] + STEP)) - total((shift[0], shift[1] - STEP))) / (2 * STEP)])
        got = WR.d_shifts(T, g, valid, shift)
        _, mag = WR.magnitudes(T, g, valid, shift)
        assert np.abs(got - want).max() <= 2e-6 * mag.max() and np.all(np.abs(got) <= mag)


# ----------------------------------------------------------------------------- the Python surface
def test_warp_checks_its_arguments_before_the_device():
    from hrnet_hip import registration
    f4, f3 = torch.zeros(2, 3, 24, 40), torch.zeros(2, 24, 40)
    with pytest.raises(TypeError, match="frames must be a torch.Tensor"):
        registration.warp(np.zeros((2, 3, 24, 40)), torch.zeros(2, 3, 2))
    with pytest.raises(ValueError, match=r"frames must be \(B,V,H,W\) or \(B,H,W\)"):
        registration.warp(torch.zeros(24, 40), torch.zeros(2))
    with pytest.raises(ValueError, match="16..16384 pixels a side"):
        registration.warp(torch.zeros(1, 1, 15, 40), torch.zeros(1, 1, 2))
    with pytest.raises(TypeError, match="shifts must be a torch.Tensor"):
        registration.warp(f4, [[0.0, 0.0]])
    with pytest.raises(ValueError, match=r"shifts must be \(B,V,2\) = \(2, 3, 2\)"):
        registration.warp(f4, torch.zeros(2, 2))
    with pytest.raises(ValueError, match=r"shifts must be \(B,2\) = \(2, 2\)"):
        registration.warp(f3, torch.zeros(2, 1, 2))
    with pytest.raises(ValueError, match="must have the shape of frames"):
        registration.warp(f4, torch.zeros(2, 3, 2), masks=torch.zeros(2, 3, 24, 41))
    with pytest.raises(TypeError, match="lr_masks must be a torch.Tensor or None"):
        registration.warp(f4, torch.zeros(2, 3, 2), masks=1.0)
    # the arguments are right: only now the device is looked at
    for frames, shifts in ((f4, torch.zeros(2, 3, 2)), (f3, torch.zeros(2, 2))):
        with pytest.raises(TypeError, match="ROCm device only"):
            registration.warp(frames, shifts)
        with pytest.raises(TypeError, match="ROCm device only"):
            registration.warp(frames.requires_grad_(True), shifts, masks=torch.ones_like(frames))


def test_ops_exist_and_state_their_schemas():
    from hrnet_hip import binding, registration  # noqa: F401
    ops = torch.ops.hrnet_hip
    assert str(ops.warp.default._schema) == "hrnet_hip::warp(Tensor views, Tensor? view_masks, Tensor shifts) -> (Tensor, Tensor)"
    assert str(ops.warp_backward.default._schema) == ("hrnet_hip::warp_backward(Tensor views, Tensor shifts, Tensor valid, Tensor d_out, "
                                                      "bool need_views, bool need_shifts) -> (Tensor, Tensor)")
    assert callable(binding.mncc_apply_backward) and "warp" in registration.__doc__ and "shift_field" in registration.__doc__
    with pytest.raises(ValueError, match="neither"):
        binding.mncc_apply_backward(torch.zeros(1, 1, 16, 16), torch.zeros(1, 1, 2), torch.zeros(1, 1, 16, 16), torch.zeros(1, 1, 16, 16),
                                    False, False)


def test_warp_bench_defaults():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import warp_bench
    o = warp_bench.PARSER.parse_args([])
    assert (o.B, o.views, o.size, o.small_batch, o.small_size, o.rounds, o.reps) == (2, 32, 512, 32, 128, 7, 5)
    o = warp_bench.PARSER.parse_args("1 --views 4 --size 64 --small-batch 2 --small-size 32 --rounds 2 --reps 1".split())
    assert (o.B, o.views, o.size, o.small_batch, o.small_size, o.rounds, o.reps) == (1, 4, 64, 2, 32, 2, 1)
    assert set(warp_bench.FAMILIES) == set(warp_bench.FLOOR_BYTES) == {"forward", "d_views", "d_shifts", "both"}
    assert warp_bench.FLOOR_BYTES["d_views"] == warp_bench.FLOOR_BYTES["d_shifts"] == 12
