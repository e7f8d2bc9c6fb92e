"""CPU: the observation model's definition on its fp64 restatement (tests/observe_ref.py) - the weights, the two forms of the matrices, the
adjoint identity, continuity across whole coordinates, the loss' analytic gradient, the range of back-projection's step, the model against
the synthetic scene, what back-projection is for - the cover of the cases (tests/observe_cases.py), and the refusals of the C ABI and of
the Python surface (hrnet_hip/observation.py), which need no device."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import observe_cases as OC
import observe_ref as O
import registration_ref as RR
import shift_add_ref as R
import shift_add_scene as SS
import upsample_ref as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- the weights and the matrices
@pytest.mark.parametrize("scale", OC.SCALES)
def test_weights_sum_to_one_and_the_tap_form_is_the_dense_form(scale):
    rng = np.random.Generator(np.random.PCG64(scale))
    for f in list(rng.uniform(0, 1, 200)) + [0.0, 0.5, 1.0 - 2.0 ** -24]:
        assert abs(O.weights_unrounded(f, scale).sum() - 1.0) <= 1e-15
    for shift in list(rng.uniform(-3.5, 3.5, 12)) + [0.0, 1.0, -2.0, 0.5, 300.0, np.nan]:
        dense, taps = O.axis_matrix(13, scale, shift), O.axis_matrix_taps(13, scale, shift)
        assert np.abs(dense - taps).max() <= 2.0 ** -24                                # the dense form holds fp32-rounded weights
        assert np.array_equal(dense != 0, np.abs(taps) > 1e-300) or np.abs(taps[dense == 0]).max() < 1e-12
        rows = dense.sum(1)
        assert np.all((np.abs(rows - 1.0) <= 4e-7) | (rows == 0))                      # constants wherever valid, nothing elsewhere
    assert not O.axis_matrix(13, scale, 300.0).any() and not O.axis_matrix(13, scale, np.nan).any()


@pytest.mark.parametrize("scale", OC.SCALES)
def test_constants_are_reproduced_wherever_valid(scale):
    rng = np.random.Generator(np.random.PCG64(10 + scale))
    shifts = rng.uniform(-2.5, 2.5, (1, 4, 2)).astype(np.float32)
    views, valid, T = O.forward(np.full((1, 11 * scale, 17 * scale), 0.625), shifts, scale)
    assert valid.any() and np.abs(views[valid] - 0.625).max() <= 1e-6 and not views[~valid].any()


@pytest.mark.parametrize("scale", OC.SCALES)
def test_adjoint_identity(scale):
    rng = np.random.Generator(np.random.PCG64(20 + scale))
    shifts = rng.uniform(-3, 3, (2, 3, 2)).astype(np.float32)
    x, r = rng.standard_normal((2, 9 * scale, 12 * scale)), rng.standard_normal((2, 3, 9, 12))
    Ax, valid, _ = O.forward(x, shifts, scale)
    Atr, _ = O.adjoint(r, shifts, scale)
    assert abs((Ax * r).sum() - (x * Atr).sum()) <= 1e-12 * np.abs(Ax * r).sum()


@pytest.mark.parametrize("scale", OC.SCALES)
def test_weights_are_continuous_across_whole_coordinates(scale):
    """f -> 1- at n equals f = 0 at n + 1: the vector at n, moved one place, is the vector at n + 1"""
    below, at = O.weights_unrounded(1.0 - 1e-9, scale), O.weights_unrounded(0.0, scale)
    assert np.abs(below[1:] - at[:-1]).max() <= 1e-7 and abs(below[0]) <= 1e-7 and abs(at[-1]) <= 1e-7
    for whole in (-2.0, 0.0, 1.0):                                     # and through the matrices: a shift just off a whole HR coordinate
        d = np.float32(whole / scale)
        lo, hi = O.axis_matrix(15, scale, np.nextafter(d, np.float32(-9))), O.axis_matrix(15, scale, np.nextafter(d, np.float32(9)))
        both = lo.any(1) & hi.any(1)
        assert both.sum() >= 8 and np.abs(lo - hi)[both].max() <= 1e-5


@pytest.mark.parametrize("brightness", [True, False])
@pytest.mark.parametrize("scale", OC.SCALES)
def test_analytic_gradient_is_the_central_difference(scale, brightness):
    rng = np.random.Generator(np.random.PCG64(30 + scale))
    B, V, H, W = 2, 3, 6, 7
    x = rng.uniform(0, 1, (B, scale * H, scale * W))
    lrs = rng.uniform(0, 1, (B, V, H, W))
    masks = (rng.uniform(0, 1, (B, V, H, W)) >= 0.3).astype(np.float32)
    alphas = np.array([[1, 0, 1], [1, 1, 1]], np.float32)
    shifts = rng.uniform(-1, 1, (B, V, 2)).astype(np.float32)
    s = O.loss(x, lrs, masks, alphas, shifts, scale, brightness)
    assert (s["n"].sum(1) > 0).all() and s["n"][0, 1] == 0
    h = 1e-5
    for _ in range(24):
        b, Y, X = rng.integers(B), rng.integers(scale * H), rng.integers(scale * W)
        xp, xm = x.copy(), x.copy()
        xp[b, Y, X] += h
        xm[b, Y, X] -= h
        num = (O.loss(xp, lrs, masks, alphas, shifts, scale, brightness)["L"][b] - O.loss(xm, lrs, masks, alphas, shifts, scale, brightness)["L"][b]) / (2 * h)
        assert abs(num - s["grad"][b, Y, X]) <= 1e-9 + 1e-6 * abs(num)


@pytest.mark.parametrize("scale", OC.SCALES)
def test_step_range_by_power_iteration(scale):
    """the largest eigenvalue of (S^2 / V) sum_v A_v^T M A_v is at most 1.02: steps in (0, 2) contract"""
    rng = np.random.Generator(np.random.PCG64(40 + scale))
    worst = 0.0
    for V in (1, 3, 9, 32):
        shape = (1, V, 10, 12)
        shifts = rng.uniform(-3.0 / scale, 3.0 / scale, (1, V, 2)).astype(np.float32) if V > 1 else np.zeros((1, 1, 2), np.float32)
        masks = (rng.uniform(0, 1, shape) >= 0.2).astype(np.float32)
        lam = O.top_eigenvalue(shape, masks, None, shifts, scale, iters=40)
        worst = max(worst, lam)
        assert 0.5 <= lam <= 1.02, (V, lam)
    print(f"x{scale}: largest eigenvalue {worst:.4f}")


# ----------------------------------------------------------------------------- the model and the scene; what back-projection is for
@pytest.mark.parametrize("scale", OC.SCALES)
def test_model_agrees_with_the_fourier_shifted_box_averaged_scene(scale):
    sc = SS.make(n_lr=48, scale=scale, views=9, band=0.25, seed=0)
    views, valid, _ = O.forward(sc["hr"][None], sc["shifts"], scale)
    cm = O.counted_map(sc["lrs"].shape, sc["masks"], None, sc["shifts"], scale)
    for v in range(9):
        d = (views - sc["lrs"])[0, v][cm[0, v]]
        rms = float(np.sqrt((d * d).mean()))
        print(f"x{scale} view {v}: rms {rms:.5f} over {d.size} counted pixels")
        assert d.size > 1000 and rms <= 1.1 * 0.005


def test_back_projection_on_the_quality_scene():
    sc = SS.make(n_lr=64, scale=3, views=9, band=0.25, limit=1.5, noise=0.005, clouds=2, margin=3.0, seed=1)
    bic = U.forward(sc["lrs"][0, 0], 3, -0.75).astype(np.float32)[None]
    start = R.forward(sc["lrs"], sc["masks"], None, sc["shifts"], 3, 0.25, 0.05, bic)[0]
    p0 = SS.psnr(start[0], sc["hr"], 12)
    x, losses = O.back_project(start, sc["lrs"], sc["masks"], None, sc["shifts"], 3, 10)
    p10 = SS.psnr(x[0], sc["hr"], 12)
    print(f"shift-and-add {p0:.2f} dB -> 10 iterations {p10:.2f} dB; data term {losses[0, 0]:.3e} -> {losses[-1, 0]:.3e}")
    assert abs(p0 - 26.28) <= 0.01 and p10 >= 32.0
    assert np.all(np.diff(losses[:, 0]) <= 0)
    ctrl, _ = O.back_project(start, sc["lrs"], sc["masks"], None, np.zeros_like(sc["shifts"]), 3, 10)
    pc = SS.psnr(ctrl[0], sc["hr"], 12)
    print(f"all shifts zero: {pc:.2f} dB")
    assert pc < p0


# ----------------------------------------------------------------------------- the cases' cover
def test_cases_cover_what_they_claim():
    plan = OC.plan()
    assert len(plan) == 126 and len({OC.case_id(c) for c in plan}) == 126
    for c in plan:
        shape, scale, kind, mkind, akind, brightness = c
        B, V, H, W = shape
        x = OC.inputs(c)
        cm = O.counted_map(shape, x["masks"], x["alphas"], x["shifts"], scale)
        for b in range(B):
            for v in range(V):
                if OC.must_count(c, x, b, v):
                    assert cm[b, v].any(), (OC.case_id(c), b, v)
        if shape in OC.DEGENERATE:
            assert not cm.any() and not O.forward(x["hr"], x["shifts"], scale)[1].any(), OC.case_id(c)
        if OC.special_view(c) is not None:
            assert not cm[:, OC.special_view(c)].any()
            if kind == "far":
                assert not O.forward(x["hr"], x["shifts"], scale)[1][:, OC.special_view(c)].any()
        if akind == "sample-zero":
            assert not cm[B - 1].any()
    for values, col in ((OC.MASKS, 3), (OC.ALPHAS, 4), ([True, False], 5)):
        for scale in OC.SCALES:
            for kind in OC.SHIFTS:
                assert {c[col] for c in plan if c[1] == scale or c[2] == kind} == set(values)


# ----------------------------------------------------------------------------- the C ABI and the Python surface refuse bad arguments
@pytest.fixture(scope="module")
def lib():
    from hrnet_hip import binding, build
    if not os.path.exists(binding.LIB_PATH):
        build.build_library(verbose=False)
    return binding.load_library()


def test_constants_agree(lib):
    from hrnet_hip import binding
    assert binding.OBSERVE_TILE == (OC.TH, OC.TW) == binding.SHIFT_ADD_TILE
    assert binding.OBSERVE_MAX_SIDE == 16384 and binding.OBSERVE_STEP == (0.0, 2.0)
    tiles = lambda B, V, H, W: B * V * -(-H // OC.TH) * -(-W // OC.TW)
    for shape in [(1, 1, 1, 1), (2, 5, 17, 63), (32, 32, 128, 128), (1, 1, 16384, 16384)]:
        assert lib.hrn_observe_workspace_bytes(*shape) == 24 * tiles(*shape)
    for shape in [(0, 1, 8, 8), (1, 0, 8, 8), (1, 1, 0, 8), (1, 1, 8, 16385), (-1, 1, 8, 8)]:
        assert lib.hrn_observe_workspace_bytes(*shape) == 0


def test_bad_arguments_fail_before_any_launch(lib):
    p, q, r, null = ctypes.c_void_p(1 << 20), ctypes.c_void_p(2 << 20), ctypes.c_void_p(3 << 20), ctypes.c_void_p(0)
    ws, st = ctypes.c_void_p(4 << 20), [ctypes.c_void_p((5 << 20) + 4096 * k) for k in range(7)]
    big = 1 << 16                                             # never dereferenced: every call below returns before a launch
    obs = lambda hr=p, shifts=q, views=r, valid=ws, B=1, V=2, H=4, W=4, scale=3: lib.hrn_observe(hr, shifts, views, valid, B, V, H, W, scale, null)
    res = lambda hr=p, lrs=q, shifts=r, residual=st[0], workspace=ws, nbytes=big, B=1, V=2, H=4, W=4, scale=3: lib.hrn_consistency_residual(
        hr, lrs, null, null, shifts, residual, workspace, nbytes, B, V, H, W, scale, null)
    fin = lambda workspace=ws, nbytes=big, o=tuple(st), B=1, V=2, H=4, W=4, scale=3, step=1.0: lib.hrn_consistency_finish(
        workspace, nbytes, *o, B, V, H, W, scale, step, 1, null)
    adj = lambda residual=p, shifts=q, out=r, x=null, B=1, V=2, H=4, W=4, scale=3: lib.hrn_observe_adjoint(
        residual, null, null, shifts, null, null, null, x, out, B, V, H, W, scale, null)
    required = ((obs, ("hr", "shifts", "views", "valid")), (res, ("hr", "lrs", "shifts", "residual", "workspace")), (fin, ("workspace",)),
                (adj, ("residual", "shifts", "out")))
    for fn, ptrs in required:
        for name in ptrs:
            assert fn(**{name: null}) == -2 and b"null" in lib.hrn_last_error(), name
        for name in ("B", "V", "H", "W"):
            assert fn(**{name: 0}) == -2 and b"empty" in lib.hrn_last_error(), name
            assert fn(**{name: -3}) == -2, name
        assert fn(H=16385) == -2 and b"16384" in lib.hrn_last_error()
        assert fn(W=16385) == -2
        for scale in (1, 5, 0):
            assert fn(scale=scale) == -2 and b"scale" in lib.hrn_last_error()
    for k in range(7):
        assert fin(o=tuple(null if i == k else s for i, s in enumerate(st))) == -2 and b"null" in lib.hrn_last_error()
    for step in (0.0, 2.0, -1.0, 2.5, float("nan"), float("inf")):
        assert fin(step=step) == -2 and b"step" in lib.hrn_last_error(), step
    # the workspace: too small, misaligned
    need = lib.hrn_observe_workspace_bytes(1, 2, 4, 4)
    assert res(nbytes=need - 1) == -2 and b"workspace" in lib.hrn_last_error()
    assert fin(nbytes=need - 1) == -2 and b"workspace" in lib.hrn_last_error()
    assert res(workspace=ctypes.c_void_p((4 << 20) + 4)) == -2 and b"aligned" in lib.hrn_last_error()
    # overlaps: only x may be out
    assert obs(views=p) == -2 and b"alias" in lib.hrn_last_error()
    assert obs(valid=r) == -2 and b"alias" in lib.hrn_last_error()
    assert res(residual=q) == -2 and b"alias" in lib.hrn_last_error()
    assert res(workspace=p) == -2 and b"alias" in lib.hrn_last_error()
    assert fin(o=(st[0], st[0]) + tuple(st[2:])) == -2 and b"alias" in lib.hrn_last_error()
    assert fin(o=(ws,) + tuple(st[1:])) == -2 and b"alias" in lib.hrn_last_error()
    assert adj(out=p) == -2 and b"alias" in lib.hrn_last_error()
    assert adj(x=ctypes.c_void_p((3 << 20) + 16)) == -2 and b"x must be" in lib.hrn_last_error()


def test_python_surface_checks_its_arguments():
    from hrnet_hip import observation
    lrs, shifts, srs = torch.zeros(2, 3, 8, 8), torch.zeros(2, 3, 2), torch.zeros(2, 24, 24)
    common = [
        (TypeError, dict(lrs=lrs.numpy())), (ValueError, dict(lrs=lrs[0])), (TypeError, dict(shifts=None)), (ValueError, dict(shifts=shifts[:, :2])),
        (ValueError, dict(lr_masks=lrs[:, :2])), (TypeError, dict(lr_masks=1.0)), (ValueError, dict(alphas=torch.ones(2, 4))),
        (ValueError, dict(scale=5)), (ValueError, dict(scale=3.0)), (ValueError, dict(scale=2)),            # srs is 24 x 24: x3 only
        (TypeError, dict(lrs=lrs.long())), (TypeError, dict(brightness=1)),
        (TypeError, dict()),                                            # everything right, but on the CPU: no fallback
    ]
    for exc, kw in common + [(TypeError, dict(srs=None)), (ValueError, dict(srs=torch.zeros(2, 24, 25))), (ValueError, dict(srs=torch.zeros(2, 2, 24, 24))),
                             (TypeError, dict(srs=torch.zeros(2, 1, 24, 24)))]:
        args = dict(srs=srs, lrs=lrs, shifts=shifts)
        args.update(kw)
        with pytest.raises(exc):
            observation.consistency_loss(**args)
    for exc, kw in common + [(ValueError, dict(sr0=torch.zeros(2, 25, 24))), (ValueError, dict(iters=-1)), (ValueError, dict(iters=2.0)),
                             (ValueError, dict(iters=True)), (ValueError, dict(step=0.0)), (ValueError, dict(step=2.0)), (ValueError, dict(step=-0.5)),
                             (ValueError, dict(step=float("nan"))), (TypeError, dict(step="big")), (TypeError, dict(step=None))]:
        args = dict(sr0=srs, lrs=lrs, shifts=shifts)
        args.update(kw)
        with pytest.raises(exc):
            observation.back_project(**args)
    for exc, kw in [(TypeError, dict(hr=None)), (ValueError, dict(hr=torch.zeros(24, 24))), (ValueError, dict(hr=torch.zeros(2, 25, 24))),
                    (ValueError, dict(shifts=torch.zeros(3, 3, 2))), (ValueError, dict(shifts=torch.zeros(2, 3))), (ValueError, dict(scale=1)),
                    (TypeError, dict(hr=srs.long())), (TypeError, dict())]:
        args = dict(hr=srs, shifts=shifts)
        args.update(kw)
        with pytest.raises(exc):
            observation.observe(**args)
    frames = torch.zeros(1, 2, 16, 16)
    with pytest.raises(ValueError, match="init"):
        observation.register_and_refine(frames, init="lanczos")
    with pytest.raises(TypeError):
        observation.register_and_refine(frames, return_trace=True)
    with pytest.raises(ValueError):
        observation.register_and_refine(frames, octaves=-1)
    with pytest.raises(ValueError):
        observation.register_and_refine(frames, step=2.0)
    for init in ("shift_add", "bicubic"):
        with pytest.raises(TypeError):                                  # the search refuses CPU tensors
            observation.register_and_refine(frames, init=init)


def test_baseline_table_takes_back_projection_and_still_refuses_the_unknown():
    from hrnet_hip import validate
    x = torch.zeros(2, 3, 16, 16)
    batch = (x, torch.ones(2, 3), torch.zeros(2, 48, 48), torch.ones(2, 48, 48), ["a", "b"])
    with pytest.raises(ValueError, match="method"):
        validate.baseline_table([batch], method="lanczos")
    with pytest.raises(TypeError, match="no further arguments"):
        validate.baseline_table([batch], iters=3)
    with pytest.raises(TypeError, match="ROCm device only"):            # everything right, but on the CPU: the search has no fallback
        validate.baseline_table([batch + (torch.ones_like(x),)], method="back_projection", iters=3)


def test_observe_bench_command_line_and_byte_floors():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import observe_bench
    o = observe_bench.PARSER.parse_args([])
    assert (o.rounds, o.reps) == (7, 10)
    assert observe_bench.CASES == [(32, 32, 128, 128, 3), (1, 32, 2048, 1536, 3)]
    lr, sr = 32 * 32 * 128 * 128, 32 * 9 * 128 * 128
    us = lambda n: 4 * n / 6.3e12 * 1e6
    assert observe_bench.floor_us(32, 32, 128, 128, 3, "residual") == pytest.approx(us(sr + 3 * lr))
    assert observe_bench.floor_us(32, 32, 128, 128, 3, "adjoint") == pytest.approx(us(2 * lr + sr))
    assert observe_bench.floor_us(32, 32, 128, 128, 3, "loss_fwd_bwd") == pytest.approx(us(sr + 3 * lr) + us(2 * lr + sr))
    assert observe_bench.floor_us(32, 32, 128, 128, 3, "iteration") == pytest.approx(us(sr + 3 * lr) + us(2 * lr + 2 * sr))
    # the tool's composition is the restatement, on the CPU in fp64
    rng = np.random.Generator(np.random.PCG64(9))
    shifts = rng.uniform(-1.5, 1.5, (2, 3, 2)).astype(np.float32)
    for scale in OC.SCALES:
        hr = rng.uniform(0, 1, (2, 8 * scale, 9 * scale))
        lrs = rng.uniform(0, 1, (2, 3, 8, 9))
        masks = (rng.uniform(0, 1, lrs.shape) >= 0.3).astype(np.float64)
        x = torch.from_numpy(hr).requires_grad_(True)
        L = observe_bench.torch_consistency_loss(x, torch.from_numpy(lrs), torch.from_numpy(masks), torch.from_numpy(shifts), scale)
        want = O.loss(hr, lrs, masks, None, shifts, scale, True)
        assert np.abs(L.detach().numpy() - want["L"]).max() <= 1e-12
        L.sum().backward()
        assert np.abs(x.grad.numpy() - want["grad"]).max() <= 1e-12
