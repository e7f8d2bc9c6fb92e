"""CPU: the shift-and-add restatement (tests/shift_add_ref.py) is what include/hrnet_hip.h defines - its own properties, the tap form
against the dense form, the cases of tests/shift_add_cases.py (their cover, and how few pixels lie at the fallback's threshold) - and
hrn_shift_add / hrn_shift_add_backward and hrnet_hip.shiftadd refuse bad arguments before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import shift_add_cases as SC
import shift_add_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kernel_is_zero_at_the_ends_of_its_support_with_zero_slope():
    for sigma in SC.SIGMAS + [0.5]:
        assert R.kernel(0.0, sigma) == 1.0
        assert R.kernel(2.0, sigma) == 0.0 and R.kernel(-2.0, sigma) == 0.0 and R.kernel(2.5, sigma) == 0.0
        u = np.array([-1.999, -0.7, 0.0, 0.3, 1.0, 1.999])
        assert (R.kernel(u, sigma) >= 0).all() and np.array_equal(R.kernel(u, sigma), R.kernel(-u, sigma))
        # cos^2(pi u / 4) = (pi / 4)^2 h^2 + O(h^4) at u = 2 - h: value and slope vanish, so a floor that falls the other way moves nothing
        for h in (1e-3, 1e-5):
            assert R.kernel(2.0 - h, sigma) <= (np.pi / 4 * h) ** 2
            assert R.kernel(-2.0 + h, sigma) <= (np.pi / 4 * h) ** 2


def test_tile_constants_agree():
    from hrnet_hip import binding
    text = open(os.path.join(ROOT, "include", "hrnet_hip.h")).read()
    th = int(re.search(r"#define HRN_SHIFT_ADD_TILE_H (\d+)", text).group(1))
    tw = int(re.search(r"#define HRN_SHIFT_ADD_TILE_W (\d+)", text).group(1))
    assert binding.SHIFT_ADD_TILE == (th, tw) == (SC.TH, SC.TW)


@pytest.mark.parametrize("scale", SC.SCALES)
def test_tap_form_is_the_dense_form_at_and_beside_whole_shifts(scale):
    """the four taps n - 1 .. n + 2 of n = floor(d) hold every non-zero of k(i - (y + d)): on whole shifts, within 1e-7 of them (where the
    fp32 d of a phase falls on either side of a whole number), on halves and at random; bit for bit, since f = d - n is exact in fp64"""
    rng = np.random.Generator(np.random.PCG64(scale))
    shifts = [0.0, 1.0, -1.0, 2.0, -2.0, 0.5, -0.5, 1.5, 300.0, -300.0, 255.9, -255.9]
    shifts += [w + e for w in (-2.0, -1.0, 0.0, 1.0, 2.0) for e in (-1e-7, 1e-7, -6e-8, 6e-8)]
    # shifts that put a phase's coordinate on a whole number: d_p = t_p + shift = whole
    shifts += [w - ((p + 0.5) / scale - 0.5) + e for w in (-1.0, 0.0, 1.0) for p in range(scale) for e in (0.0, -1e-7, 1e-7)]
    shifts += list(rng.uniform(-3.5, 3.5, 20))
    for sigma in SC.SIGMAS:
        for n in (1, 2, 5, 9):
            for s in shifts:
                dense, tap = R.axis_matrix(n, scale, s, sigma), R.axis_matrix_taps(n, scale, s, sigma)
                assert np.array_equal(dense, tap), (scale, sigma, n, s)
    # the phases of a view read among five consecutive indices: n_p is n_0 or n_0 + 1
    for s in shifts:
        nn, w = R.taps(s, scale, 0.25)
        assert ((nn - nn[0] >= 0) & (nn - nn[0] <= 1)).all() and (w >= 0).all()
    assert not R.axis_matrix(4, scale, np.nan, 0.25).any() and not R.axis_matrix(4, scale, np.inf, 0.25).any()


def test_coordinates_are_clamped_and_weights_are_fp32_or_zero():
    assert np.array_equal(R.tap_coord(300.0, 3), np.float32([256, 256, 256])) and np.array_equal(R.tap_coord(-300.0, 2), np.float32([-256, -256]))
    assert np.array_equal(R.axis_matrix(3, 3, 300.0, 0.25), R.axis_matrix(3, 3, 256.0, 0.25))
    for sigma in SC.SIGMAS:
        _, w = R.taps(0.37, 4, sigma)
        assert np.array_equal(w, w.astype(np.float32).astype(np.float64))
        assert ((w == 0) | (w >= R.MIN_TAP)).all()
    # at sigma = 0.1 the far taps fall under 2^-60 and are dropped: no product of two kept weights is a subnormal fp32 number
    _, w = R.taps(0.0, 2, 0.1)
    assert (w == 0).any() and float(w[w > 0].min()) ** 2 >= 2.0 ** -126


@pytest.mark.parametrize("scale", SC.SCALES)
def test_constant_views_give_the_constant_wherever_a_sample_reaches(scale):
    """the partition of unity of a normalised convolution: with prior 0, N = c D"""
    rng = np.random.Generator(np.random.PCG64(10 + scale))
    B, V, H, W = 2, 3, 6, 7
    views = np.full((B, V, H, W), 0.625, np.float32)
    masks = (rng.uniform(0, 1, views.shape) >= 0.5).astype(np.float32)
    shifts = rng.uniform(-2, 2, (B, V, 2)).astype(np.float32)
    for sigma in SC.SIGMAS:
        out, D, T, den = R.forward(views, masks, None, shifts, scale, sigma, 0.0)
        ok = den >= R.MIN_DEN
        assert ok.any() and np.abs(out[ok] - 0.625).max() <= 1e-12
        assert not out[~ok].any()
        # with a base and a prior the result lies between the constant and the base
        base = np.full(out.shape, 0.125, np.float32)
        out2 = R.forward(views, masks, None, shifts, scale, sigma, 0.05, base)[0]
        assert (out2 >= 0.125 - 1e-12).all() and (out2 <= 0.625 + 1e-12).all()


def test_adjoint_identity_and_the_skipped_views_of_the_restatement():
    rng = np.random.Generator(np.random.PCG64(3))
    B, V, H, W, scale, sigma, prior = 2, 4, 5, 6, 3, 0.25, 0.05
    views = rng.uniform(-1, 1, (B, V, H, W)).astype(np.float32)
    masks = (rng.uniform(0, 1, views.shape) >= 0.3).astype(np.float32)
    alphas = np.array([[1, 0, 1, 1], [1, 1, 0.5, 0]], np.float32)
    shifts = rng.uniform(-2.5, 2.5, (B, V, 2)).astype(np.float32)
    shifts[0, 2, 0] = np.nan
    base = rng.uniform(-1, 1, (B, scale * H, scale * W)).astype(np.float32)
    g = rng.uniform(-1, 1, base.shape).astype(np.float32)
    out, D, T, den = R.forward(views, masks, alphas, shifts, scale, sigma, prior, base)
    dv, Tv, db, Tb = R.adjoint(g, D.astype(np.float32), masks, alphas, shifts, V, H, W, scale, sigma, prior)
    # out is linear in (views, base): <out, g> = <views, d_views> + <base, d_base> (weight went through fp32: a relative 1e-7)
    lhs, rhs = float((out * g).sum()), float((views * dv).sum() + (base * db).sum())
    assert abs(lhs - rhs) <= 1e-6 * float((T * np.abs(g)).sum())
    assert not dv[0, 1].any() and not dv[1, 3].any() and not dv[0, 2].any() and dv[1, 2].any()
    assert not dv[masks == 0].any()
    # appended alpha-0 views and a view with a non-finite shift change nothing
    views2 = np.concatenate([views, rng.uniform(-1, 1, (B, 2, H, W)).astype(np.float32)], 1)
    pad = lambda t, v: np.concatenate([t, np.full((B, 2) + t.shape[2:], v, np.float32)], 1)
    out2 = R.forward(views2, pad(masks, 1), pad(alphas, 0), pad(shifts, 0.3), scale, sigma, prior, base)[0]
    assert np.array_equal(out, out2)


def test_forward_is_continuous_across_whole_shifts():
    """a floor that falls the other way moves nothing: the results on both sides of a whole coordinate differ by O(eps)"""
    rng = np.random.Generator(np.random.PCG64(4))
    views = rng.uniform(0, 1, (1, 2, 6, 6)).astype(np.float32)
    for scale in SC.SCALES:
        for whole in (-1.0, 0.0, 2.0):
            for p in range(scale):
                s0 = whole - ((p + 0.5) / scale - 0.5)
                res = []
                for e in (-2e-6, 2e-6):
                    shifts = np.zeros((1, 2, 2), np.float32)
                    shifts[0, 1] = (s0 + e, s0 - e)
                    res.append(R.forward(views, None, None, shifts, scale, 0.25, 0.0)[0])
                assert np.abs(res[0] - res[1]).max() <= 1e-4


def test_the_plan_covers_every_value_with_every_scale_and_kind_of_shift():
    plan = SC.plan()
    assert len(plan) == len(set(plan)) == len(SC.SHAPES) * len(SC.SCALES) * len(SC.SHIFTS)
    for pos, values in ((3, SC.SIGMAS), (4, SC.PRIORS), (5, SC.MASKS), (6, SC.ALPHAS)):
        for v in values:
            with_v = [c for c in plan if c[pos] == v]
            assert {c[1] for c in with_v} == set(SC.SCALES), (pos, v)
            assert {c[2] for c in with_v} == set(SC.SHIFTS), (pos, v)
            assert {c[0] for c in with_v} == set(SC.SHAPES), (pos, v)


def test_few_pixels_of_a_case_lie_at_the_threshold_and_block_cases_have_exact_zeros():
    """the pixels whose D + prior lies in [2^-21, 2^-19] are left out of the device comparison: at most 0.1 % of a case's pixels; and
    the block masks leave pixels no sample reaches (D exactly 0) beside pixels that samples reach"""
    worst, zeros = 0.0, 0
    for c in SC.plan():
        ref = SC.reference(c)
        frac = 1.0 - float(ref["keep"].mean())
        worst = max(worst, frac)
        assert frac <= 1e-3, (SC.case_id(c), frac)
        if c[5] == "block" and (ref["D"] == 0).any() and (ref["D"] > 0).any():
            zeros += 1
    print(f"largest share of excluded pixels {worst:.2e}; block cases with exact zeros beside reached pixels: {zeros}")
    assert zeros >= 6


# ----------------------------------------------------------------------------- the C ABI and the Python surface refuse bad arguments
@pytest.fixture(scope="module")
def lib():
    from hrnet_hip import binding, build
    if not os.path.exists(binding.LIB_PATH):
        build.build_library(verbose=False)
    return binding.load_library()


def test_bad_arguments_fail_before_any_launch(lib):
    p, null = ctypes.c_void_p(4096), ctypes.c_void_p(0)       # never dereferenced: every call below returns before a launch
    fwd = lambda views=p, shifts=p, out=p, B=1, V=2, H=4, W=4, scale=3, sigma=0.25, prior=0.05: lib.hrn_shift_add(
        views, null, null, shifts, null, out, null, B, V, H, W, scale, sigma, prior, null)
    bwd = lambda d_out=p, weight=p, shifts=p, B=1, V=2, H=4, W=4, scale=3, sigma=0.25, prior=0.05: lib.hrn_shift_add_backward(
        d_out, weight, null, null, shifts, null, null, B, V, H, W, scale, sigma, prior, null)
    for fn, ptrs in ((fwd, ("views", "shifts", "out")), (bwd, ("d_out", "weight", "shifts"))):
        for name in ptrs:
            assert fn(**{name: null}) == -2 and b"null" in lib.hrn_last_error(), name
        for name in ("B", "V", "H", "W"):
            assert fn(**{name: 0}) == -2 and b"empty" in lib.hrn_last_error(), name
            assert fn(**{name: -3}) == -2, name
        assert fn(H=16385) == -2 and b"16384" in lib.hrn_last_error()
        assert fn(W=16385) == -2
        for scale in (1, 5, 0):
            assert fn(scale=scale) == -2 and b"scale" in lib.hrn_last_error()
        for sigma in (0.05, 1.5, 0.0, -0.25, float("nan"), float("inf")):
            assert fn(sigma=sigma) == -2 and b"sigma" in lib.hrn_last_error(), sigma
        for prior in (-0.1, float("nan"), float("inf")):
            assert fn(prior=prior) == -2 and b"prior" in lib.hrn_last_error(), prior
    # base may be out itself and nothing else may overlap an output
    assert lib.hrn_shift_add(p, null, null, p, null, p, null, 1, 2, 4, 4, 3, 0.25, 0.05, null) == -2 and b"alias" in lib.hrn_last_error()
    q = ctypes.c_void_p(1 << 20)
    assert lib.hrn_shift_add(p, null, null, p, ctypes.c_void_p((1 << 20) + 16), q, null, 1, 2, 4, 4, 3, 0.25, 0.05, null) == -2
    assert b"base" in lib.hrn_last_error()
    assert lib.hrn_shift_add(p, null, null, p, null, q, q, 1, 2, 4, 4, 3, 0.25, 0.05, null) == -2 and b"weight" in lib.hrn_last_error()
    assert lib.hrn_shift_add_backward(q, p, null, null, p, q, null, 1, 2, 4, 4, 3, 0.25, 0.05, null) == -2 and b"d_views" in lib.hrn_last_error()
    assert lib.hrn_shift_add_backward(q, p, null, null, p, null, q, 1, 2, 4, 4, 3, 0.25, 0.05, null) == -2 and b"d_base" in lib.hrn_last_error()


def test_python_surface_checks_its_arguments():
    from hrnet_hip import shiftadd
    lrs, shifts = torch.zeros(2, 3, 8, 8), torch.zeros(2, 3, 2)
    bad = [
        (TypeError, dict(lrs=lrs.numpy())), (ValueError, dict(lrs=lrs[0])), (TypeError, dict(shifts=None)), (ValueError, dict(shifts=shifts[:, :2])),
        (ValueError, dict(lr_masks=lrs[:, :2])), (TypeError, dict(lr_masks=1.0)), (ValueError, dict(alphas=torch.ones(2, 4))),
        (ValueError, dict(scale=5)), (ValueError, dict(scale=3.0)), (ValueError, dict(sigma=0.05)), (ValueError, dict(sigma=1.01)),
        (TypeError, dict(sigma="wide")), (ValueError, dict(sigma=float("nan"))), (ValueError, dict(prior=-1e-3)), (TypeError, dict(prior=None)),
        (ValueError, dict(base=None)),                                  # with the default prior
        (ValueError, dict(base="lanczos")), (TypeError, dict(base=3)), (ValueError, dict(base=torch.zeros(2, 24, 25))),
        (TypeError, dict(lrs=lrs.long())),
        (TypeError, dict()),                                            # everything right, but on the CPU: no fallback
        (TypeError, dict(base=None, prior=0)),
    ]
    for exc, kw in bad:
        args = dict(lrs=lrs, shifts=shifts)
        args.update(kw)
        with pytest.raises(exc):
            shiftadd.shift_and_add(**args)
    with pytest.raises(TypeError):
        shiftadd.register_and_add(torch.zeros(1, 2, 16, 16), return_trace=True)
    with pytest.raises(ValueError):
        shiftadd.register_and_add(torch.zeros(1, 2, 16, 16), octaves=-1)
    with pytest.raises(TypeError):                                      # the search refuses CPU tensors
        shiftadd.register_and_add(torch.zeros(1, 2, 16, 16))


def test_baseline_table_method_and_the_sixth_batch_item():
    from hrnet_hip import validate
    x = torch.zeros(2, 3, 16, 16)
    batch = (x, torch.ones(2, 3), torch.zeros(2, 48, 48), torch.ones(2, 48, 48), ["a", "b"])
    with pytest.raises(ValueError, match="method"):
        validate.baseline_table([batch], method="lanczos")
    with pytest.raises(TypeError, match="no further arguments"):
        validate.baseline_table([batch], sigma=0.3)
    with pytest.raises(ValueError, match="names"):                     # a sixth item is a batch; its names are still counted
        validate.baseline_table([batch[:4] + (["only-one"], torch.ones_like(x))], method="shift_add")
    with pytest.raises(ValueError, match="7 elements"):
        validate.baseline_table([batch + (x, x)])
    with pytest.raises(TypeError, match="ROCm device only"):            # everything right, but on the CPU: the search has no fallback
        validate.baseline_table([batch + (torch.ones_like(x),)], method="shift_add")


def test_shift_add_bench_command_line_and_byte_floors():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import shift_add_bench
    o = shift_add_bench.PARSER.parse_args([])
    assert (o.rounds, o.reps) == (7, 10)
    assert shift_add_bench.CASES == [(32, 32, 128, 128, 3), (1, 32, 2048, 1536, 3)]
    lr, sr = 32 * 32 * 128 * 128, 32 * 9 * 128 * 128
    assert shift_add_bench.floor_us(32, 32, 128, 128, 3, "forward") == pytest.approx(4 * (2 * lr + 2 * sr) / 6.3e12 * 1e6)
    assert shift_add_bench.floor_us(32, 32, 128, 128, 3, "forward_weight") == pytest.approx(4 * (2 * lr + 3 * sr) / 6.3e12 * 1e6)
    assert shift_add_bench.floor_us(32, 32, 128, 128, 3, "backward") == pytest.approx(4 * (2 * lr + 3 * sr) / 6.3e12 * 1e6)
    # the tool's composition is the restatement: taps and, on the CPU in fp32, the whole definition
    rng = np.random.Generator(np.random.PCG64(9))
    shifts = rng.uniform(-2.5, 2.5, (2, 3, 2)).astype(np.float32)
    shifts[1, 2, 0] = np.nan
    for scale in SC.SCALES:
        n, w = shift_add_bench.taps(torch.from_numpy(shifts[0, :, 0]), scale, 0.25)
        for v in range(3):
            nn, ww = R.taps(shifts[0, v, 0], scale, 0.25)
            assert np.array_equal(n[v].numpy(), nn) and np.array_equal(w[v].double().numpy(), ww)
        views = rng.uniform(0, 1, (2, 3, 6, 9)).astype(np.float32)
        masks = (rng.uniform(0, 1, views.shape) >= 0.3).astype(np.float32)
        alphas = np.array([[1, 1, 0], [1, 1, 1]], np.float32)
        base = rng.uniform(0, 1, (2, 6 * scale, 9 * scale)).astype(np.float32)
        out, D = shift_add_bench.torch_shift_add(*(torch.from_numpy(a) for a in (views, masks, alphas, shifts, base)), scale, 0.25, 0.05)
        want, Dw, T, den = R.forward(views, masks, alphas, shifts, scale, 0.25, 0.05, base)
        assert np.abs(out.double().numpy() - want).max() <= 1e-5 and np.abs(D.double().numpy() - Dw).max() <= 1e-5 * Dw.max()
