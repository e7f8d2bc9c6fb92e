"""CPU: the sub-pixel searched cMSE / cPSNR loss on its fp64 restatement, tests/subpixel_ref.py - that the search
scored by the brightness-corrected cMSE recovers known sub-pixel shifts, far from a tie at every level, and pays off against the best
whole-pixel offset; that the six-sum formula the kernels keep is the direct cMSE; that the restated gradient is the derivative of the
restated loss with the shift held - and the C entry points' refusals, which need no device (the pointers below are never dereferenced).

The scenes are the issue's: registration_ref._parts(H, W, shifts, seed), target 0.3 + 0.1 z, prediction 0.33 + 0.1 z_shifted + 0.002 N, at
(24, 40) seed 1, (70, 83) seed 2, (130, 203) seed 3, each with the true shifts (0.37, -0.62), (2, 0), (-2.4, 1.55), (0, 0), (2.9, -2.9);
P = 7, 4 levels, radius 3, border 3.  A last-level step is 2 * 3 * 0.25^3 / 6 = 0.015625 px: half a step of quantisation plus the noise.
Measured on the restatement: every shift within 0.0094 px, the top-two gap at least 9.0e-3 at every level."""
import ctypes
import os

import numpy as np
import pytest

import subpixel_ref as SP

CASES = [(shape, seed, shift) for shape, seed in SP.SHAPES for shift in SP.SHIFTS]
IDS = [f"{h}x{w}-{dy:g},{dx:g}" for (h, w), _, (dy, dx) in CASES]
_found = {}


def found(shape, seed, shift):
    """the scene and its search, once per case"""
    key = (shape, seed, shift)
    if key not in _found:
        x = SP.scene(*shape, shift, seed)
        _found[key] = (x, SP.search(*x))
    return _found[key]


@pytest.mark.parametrize("shape,seed,shift", CASES, ids=IDS)
def test_search_recovers_the_shift_far_from_a_tie(shape, seed, shift):
    x, s = found(shape, seed, shift)
    err = np.abs(s["shift"].astype(np.float64) - np.array(shift))
    print(f"shift error {err.max():.4f} px, gaps {s['gaps']}, cMSE* {s['cmse']:.3e}")
    assert err.max() <= SP.LAST_STEP
    assert s["gaps"].min() >= 5e-3
    whole = min(SP.cmse(*x, SP.BORDER, (float(u), float(v)))[0] for u in range(-3, 4) for v in range(-3, 4))
    print(f"best whole-pixel cMSE {whole:.3e}")
    assert s["cmse"] <= whole
    if any(float(d) != round(d) for d in shift):
        assert s["cmse"] < 0.1 * whole
    assert s["n"] == SP.residual(*x, SP.BORDER, s["shift"])[1] > 0


@pytest.mark.parametrize("shape,seed,shift", CASES[::2], ids=IDS[::2])
def test_six_sums_are_the_direct_cmse(shape, seed, shift):
    x, s = found(shape, seed, shift)
    sr, hr, hr_map = x
    m0 = SP.crop_mask(hr_map, SP.BORDER)
    means = (float(np.float32(sr.astype(np.float64).mean())), float(np.float32(hr.astype(np.float64)[m0].mean())))
    for at in (s["shift"], (0.0, 0.0), s["coords"][0][:, 1], s["coords"][2][:, 5]):
        want, n, b = SP.cmse(*x, SP.BORDER, at)
        got, centred, n6 = SP.six_sums(*x, SP.BORDER, at, *means)          # on images centred by their whole-frame means, as the kernels
        plain = SP.six_sums(*x, SP.BORDER, at, *means, dtype=np.float64)[0]
        print(f"six sums vs direct: {abs(got - want) / want:.2e} relative; evaluated in float64 {abs(plain - want) / want:.2e}")
        assert abs(plain - want) <= 2.0 ** -50 * 0.02                    # float64: 4 roundings of the mean of t^2 + r^2, at most 0.02 here
        assert n6 == n and abs(got - want) <= 1e-12 * want
        assert abs(centred + (means[1] - means[0]) - b) <= 1e-12


@pytest.mark.parametrize("metric", ["cMSE", "cPSNR"])
@pytest.mark.parametrize("shape,seed,shift", [CASES[0], CASES[7], CASES[14]], ids=[IDS[0], IDS[7], IDS[14]])
def test_gradient_is_the_central_difference_with_the_shift_held(shape, seed, shift, metric):
    x, s = found(shape, seed, shift)
    sr, hr, hr_map = (np.asarray(a, np.float64) for a in x)
    at = s["shift"]
    g = SP.grad(sr, hr, hr_map, SP.BORDER, at, metric)
    rng = np.random.default_rng(seed)
    H, W = shape
    pixels = [(0, 0), (H - 1, W - 1), (SP.BORDER, SP.BORDER), (H // 2, W // 2)] + [(int(rng.integers(H)), int(rng.integers(W))) for _ in range(8)]
    # cPSNR's truncation error is c2 h^2 / cMSE relative, c2 <= 1 / n, and its rounding error 54 * 2^-53 / (2 h |g|) with |g| ~ 1 / n:
    # h grows with sqrt(n) to keep both below 2e-7 on every shape
    h = 1e-5 * (s["n"] / 448.0) ** 0.5
    for y, x_ in pixels:
        d = np.zeros((H, W))
        d[y, x_] = h
        lo, hi = (SP.loss_of(SP.cmse(sr + sign * d, hr, hr_map, SP.BORDER, at)[0], metric) for sign in (-1.0, 1.0))
        want = (hi - lo) / (2 * h)
        assert abs(g[y, x_] - want) <= 1e-6 * max(abs(want), np.abs(g).max() * 1e-3), (y, x_, g[y, x_], want)
    assert g[0, 0] == 0.0 and np.abs(g).max() > 0.0


def test_controls_change_the_restatement():
    x, s = found(*CASES[12])                                       # (130, 203), (-2.4, 1.55)
    base = SP.grad(*x, SP.BORDER, s["shift"], "cPSNR")
    for name in SP.CONTROLS:
        other = SP.grad(*x, SP.BORDER, s["shift"], "cPSNR", **{name: True})
        assert np.abs(other - base).max() > 1e-3 * np.abs(base).max(), name


# ----------------------------------------------------------------------------- the C ABI, without a device
@pytest.fixture(scope="module")
def lib():
    from hrnet_hip import binding, build
    if not os.path.exists(binding.LIB_PATH):
        build.build_library(verbose=False)
    return binding.load_library()


B, H, W = 2, 70, 83
NULL = ctypes.c_void_p(0)


def _train(lib, p, **kw):
    a = dict(srs=p, hrs=p, maps=p, B=B, H=H, W=W, border=3, P=7, levels=4, radius=3.0, metric=2, out=p, stats=p, trace=p, ws=p,
             ws_bytes=lib.hrn_subpixel_loss_workspace_bytes(B, H, W, 7), stream=NULL)
    a.update(kw)
    return lib.hrn_subpixel_loss_train(a["srs"], a["hrs"], a["maps"], a["B"], a["H"], a["W"], a["border"], a["P"], a["levels"], a["radius"],
                                       a["metric"], a["out"], a["stats"], a["trace"], a["ws"], a["ws_bytes"], a["stream"])


def _backward(lib, p, **kw):
    a = dict(srs=p, hrs=p, maps=p, stats=p, d_out=p, B=B, H=H, W=W, border=3, metric=2, d_srs=p, ws=p,
             ws_bytes=lib.hrn_subpixel_loss_workspace_bytes(B, H, W, 3), stream=NULL)
    a.update(kw)
    return lib.hrn_subpixel_loss_backward(a["srs"], a["hrs"], a["maps"], a["stats"], a["d_out"], a["B"], a["H"], a["W"], a["border"],
                                          a["metric"], a["d_srs"], a["ws"], a["ws_bytes"], a["stream"])


def test_abi_is_declared_and_built(lib):
    from hrnet_hip import binding, build, losses
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "hrnet_hip.h")).read()
    for n in ("hrn_subpixel_loss_workspace_bytes", "hrn_subpixel_loss_train", "hrn_subpixel_loss_backward"):
        assert n in binding.SIGNATURES and hasattr(lib, n) and n + "(" in header, n
    assert "subpixel_loss.hip" in build.SOURCES and callable(losses.subpixel_loss)


def test_workspace_bytes(lib):
    def want(b, h, w, p):
        plane = (4 * b * h * w + 15) // 16 * 16
        tiles, chunks = -(-h // 64) * -(-w // 64), min(64, -(-h * w // 16384))
        return max(plane + 16 * 2 * b * chunks + 48 * p * p * b * tiles + 8 * b, 2 * plane + 8 * b)
    for args in ((1, 24, 40, 7), (2, 70, 83, 7), (1, 130, 203, 9), (3, 17, 19, 3), (2, 16, 16, 9)):
        assert lib.hrn_subpixel_loss_workspace_bytes(*args) == want(*args)
    for bad in ((0, H, W, 7), (B, 15, W, 7), (B, H, 16385, 7), (B, H, W, 2), (B, H, W, 10)):
        assert lib.hrn_subpixel_loss_workspace_bytes(*bad) == 0


def test_bad_arguments_fail_before_any_launch(lib):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    for name in ("srs", "hrs", "maps", "out", "stats", "ws"):
        assert _train(lib, p, **{name: NULL}) == -2 and b"null" in lib.hrn_last_error()
    for name in ("srs", "hrs", "maps", "stats", "d_out", "d_srs", "ws"):
        assert _backward(lib, p, **{name: NULL}) == -2 and b"null" in lib.hrn_last_error()
    for call in (_train, _backward):
        assert call(lib, p, border=9) == -2 and b"border" in lib.hrn_last_error()
        assert call(lib, p, border=-1) == -2
        assert call(lib, p, H=16, border=8) == -2 and b"half" in lib.hrn_last_error()
        assert call(lib, p, H=15) == -2 and b"sides" in lib.hrn_last_error()
        assert call(lib, p, W=16385) == -2
        assert call(lib, p, B=0) == -2
        assert call(lib, p, B=2 ** 20, H=16384, W=16384) == -2 and b"one launch" in lib.hrn_last_error()      # B T beyond 2^31 - 1
        assert call(lib, p, metric=0) == -2 and b"metric" in lib.hrn_last_error()
    assert _train(lib, p, P=2) == -2 and b"points" in lib.hrn_last_error()
    assert _train(lib, p, P=10) == -2
    assert _train(lib, p, levels=0) == -2 and b"levels" in lib.hrn_last_error()
    assert _train(lib, p, levels=17) == -2
    for radius in (0.0, -1.0, 4.5, float("nan")):
        assert _train(lib, p, radius=radius) == -2 and b"radius" in lib.hrn_last_error()
    assert _train(lib, p, trace=NULL, ws_bytes=lib.hrn_subpixel_loss_workspace_bytes(B, H, W, 7) - 1) == -3 and b"workspace" in lib.hrn_last_error()
    assert _train(lib, p, ws_bytes=0) == -3
    assert _backward(lib, p, ws_bytes=8 * B * H * W) == -3 and b"workspace" in lib.hrn_last_error()


def test_wrapper_checks_arguments_before_the_device():
    import torch
    from hrnet_hip import losses
    x = torch.zeros(2, 24, 40)
    for kw, text in ((dict(metric="masked_MSE"), "metric"), (dict(points_per_dim=2), "points_per_dim"), (dict(levels=0), "levels"),
                     (dict(radius=0.0), "radius"), (dict(radius=5.0), "radius"), (dict(border_w=9), "border_w")):
        with pytest.raises(ValueError, match=text):
            losses.subpixel_loss(x, x, x, **kw)
    with pytest.raises(ValueError, match="sides"):
        losses.subpixel_loss(x[:, :15], x[:, :15], x[:, :15])
    with pytest.raises(ValueError, match="equal"):
        losses.subpixel_loss(x, x[:1], x)
    with pytest.raises(TypeError, match="torch.Tensor"):
        losses.subpixel_loss(x.numpy(), x, x)
    with pytest.raises(TypeError, match="no CPU fallback"):          # the device last
        losses.subpixel_loss(x[:, None], x, x)
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import train_step_bench
    o = vars(train_step_bench.options("32 32 64 10 --precision bf16 --loss shift,subpixel --repeats 3".split()))
    assert o["loss"] == ["shift", "subpixel"] and "subpixel" in train_step_bench.SEARCHED
    import shift_loss_bench
    assert {"subpixel_fwd", "subpixel_bwd"} <= set(shift_loss_bench.SUBPIXEL)
