"""CPU: the fp64 restatement of the masked-NCC registration search (tests/registration_ref.py) recovers the known
shifts of synthetic scenes and behaves at its edges; the C entry points refuse bad arguments before any launch; hrnet_hip.registration
checks its arguments; the fake kernels give the right shapes.  Nothing here needs a GPU."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import registration_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(16, 16), (24, 40), (33, 47), (64, 64)]
RECOVERY_PX = 0.02           # the issue's bound on every component of a recovered shift


@functools.lru_cache(maxsize=None)
def scene(H, W, limit=0.9, V=4):
    shifts = R.random_shifts(V, limit, seed=1000 + H * W)
    return (shifts,) + R.scene(H, W, shifts, seed=H * W)


# ----------------------------------------------------------------------------- the restatement itself
@pytest.mark.parametrize("P,levels", [(7, 5), (5, 6)], ids=["P7_L5", "P5_L6"])
@pytest.mark.parametrize("H,W", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_restatement_recovers_known_shifts(H, W, P, levels):
    shifts, ref, ref_mask, views, view_masks = scene(H, W)
    for v in range(len(shifts)):
        got, trace = R.search(ref, ref_mask, views[v], view_masks[v], P, levels, 1.0)
        err = np.abs(got.astype(np.float64) - shifts[v])
        print(f"{H}x{W} P={P} view {v}: true {shifts[v]}, found {got}, error {err.max():.4f} px, score {trace[-1, 2]:.6f}")
        assert err.max() <= RECOVERY_PX
        assert np.all(np.diff(trace[:, 2]) >= 0.0) and trace[-1, 2] <= 1.0       # a level holds its centre, so the score never falls
        assert np.array_equal(trace[-1, :2], got.astype(np.float64))


def test_restatement_recovers_larger_shifts_with_radius_2():
    shifts, ref, ref_mask, views, view_masks = scene(33, 47, limit=1.8, V=2)
    for v in range(len(shifts)):
        got, _ = R.search(ref, ref_mask, views[v], view_masks[v], 7, 5, 2.0)
        assert np.abs(got - shifts[v]).max() <= RECOVERY_PX


def test_three_points_per_axis_give_a_valid_search():
    """P = 3 narrows by 0.9 a level: run for validity, not accuracy."""
    shifts, ref, ref_mask, views, view_masks = scene(16, 16)
    got, trace = R.search(ref, ref_mask, views[0], view_masks[0], 3, 4, 1.0)
    assert np.all(np.isfinite(trace)) and np.all(np.abs(got) <= 1.0 + 0.9 + 0.81 + 0.729)
    assert np.all(np.diff(trace[:, 2]) >= 0.0) and np.all(np.abs(trace[:, 2]) <= 1.0)
    assert R.level_widths(3, 3, 1.0) == [2.0, 2.0 * 0.9, 2.0 * 0.9 * 0.9]
    assert R.level_widths(4, 2, 1.0) == [2.0, 1.0] and R.level_widths(9, 2, 0.5) == [1.0, 0.25]


def test_identical_frames_score_one_at_zero_shift():
    _, ref, _, _, _ = scene(24, 40)
    assert abs(R.score(ref, None, ref, None, (0.0, 0.0)) - 1.0) <= 1e-12
    ones = np.ones_like(ref)
    assert abs(R.score(ref, ones, ref, ones, (0.0, 0.0)) - 1.0) <= 1e-12
    s, dys, dxs = R.grid(ref, None, ref, None, (0.0, 0.0), 2.0, 7)
    assert R.best_of(s, dys, dxs, (0.0, 0.0))[0] == (0.0, 0.0) and np.all(s <= 1.0)


def test_sampler_and_mask_follow_the_shift_convention():
    """Output(y, x) = Input(y + dy, x + dx); whole-pixel shifts are exact, the footprint frame is zero and invalid."""
    rng = np.random.default_rng(3)
    T = rng.random((16, 20))
    out = R.sample(T, (2.0, -3.0))
    inside = R.inside(T.shape, (2.0, -3.0))
    assert np.array_equal(np.argwhere(inside)[[0, -1]], [[0, 5], [10, 19]])          # rows y + 2 - 2 >= 0 .. y + 2 + 3 <= 15, columns x - 3 - 2 >= 0
    assert np.allclose(out[inside], np.roll(T, (-2, 3), (0, 1))[inside], rtol=0, atol=1e-15) and np.all(out[~inside] == 0.0)
    assert abs(R.taps(0.37).sum() - 1.0) < 1e-15 and np.allclose(R.taps(0.0), [0, 0, 1, 0, 0, 0], rtol=0, atol=1e-16)
    a, b = R.sample(T, (np.float32(0.5) - np.float32(1e-6), 0.25)), R.sample(T, (np.float32(0.5) + np.float32(1e-6), 0.25))
    assert np.abs(a - b).max() < 1e-5                                                # continuous across the half pixel
    a, b = R.sample(T, (np.float32(1.0) - np.float32(1e-6), 0.25)), R.sample(T, (1.0, 0.25))
    both = R.inside(T.shape, (0.5, 0.25)) & R.inside(T.shape, (1.0, 0.25))
    assert np.abs(a - b)[both].max() < 1e-5                                          # and across the whole pixel
    M = np.ones((16, 20))
    M[4:8, 6:9] = 0.0
    v = R.mask_bilinear(M, (0.5, 0.0))
    assert v[3, 7] == 0.5 and v[2, 7] == 1.0 and v[4, 7] == 0.0 and not R.shifted_mask(M, (0.5, 0.0))[3, 7]
    assert R.mask_bilinear(M, (0.0, -1.0))[5, 9] == 0.0 and R.mask_bilinear(M, (0.0, -1.0))[5, 10] == 1.0
    assert R.mask_bilinear(M, (0.25, 0.0))[15, 3] == 0.75                            # zeros beyond the frame


def test_an_empty_view_scores_minus_infinity_and_keeps_the_centre():
    _, ref, ref_mask, views, view_masks = scene(16, 16)
    for view, mask in ((np.zeros_like(views[0]), view_masks[0]), (views[0], np.zeros_like(view_masks[0]))):
        assert R.score(ref, ref_mask, view, mask, (0.0, 0.0)) == -np.inf
        got, trace = R.search(ref, ref_mask, view, mask, 7, 3, 1.0)
        assert np.array_equal(got, [0.0, 0.0]) and np.all(trace[:, :2] == 0.0) and np.all(trace[:, 2] == -np.inf)
    assert R.score(ref, np.zeros_like(ref_mask), views[0], view_masks[0], (0.25, 0.5)) == -np.inf
    assert R.score(ref, ref_mask, views[0], view_masks[0], (40.0, 0.0)) == -np.inf   # no footprint inside the frame


# ----------------------------------------------------------------------------- the new surface, host side
NAMES = ("hrn_mncc_grid", "hrn_mncc_search", "hrn_mncc_apply")


@pytest.fixture(scope="module")
def lib():
    from hrnet_hip import binding, build
    if not os.path.exists(binding.LIB_PATH):
        build.build_library(verbose=False)
    return binding.load_library()


def test_exports_are_present(lib):
    import hrnet_hip
    from hrnet_hip import binding, build, registration
    header = open(os.path.join(ROOT, "include", "hrnet_hip.h")).read()
    for n in NAMES:
        assert n in binding.SIGNATURES and hasattr(lib, n) and n + "(" in header, n
    assert "registration.hip" in build.SOURCES and hrnet_hip.registration is registration
    for f in ("mncc_search", "mncc_grid", "shift_views", "register_views"):
        assert callable(getattr(registration, f))
    for f in ("mncc_grid", "mncc_search", "mncc_apply"):
        assert callable(getattr(binding, f))
    for op in ("mncc_grid", "mncc_search", "shift_views"):
        assert hasattr(torch.ops.hrnet_hip, op)


def test_c_entry_points_refuse_bad_arguments_before_any_launch(lib):
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(64)          # p: never dereferenced, every call below fails its checks first

    def grid(H=16, W=16, P=7, width=2.0, a=p, B=2, V=3):
        return lib.hrn_mncc_grid(a, p, p, p, p, B, V, H, W, P, width, p, null)

    def search(H=16, W=16, P=7, levels=6, radius=1.0, a=p, B=2, V=3):
        return lib.hrn_mncc_search(a, p, p, p, B, V, H, W, P, levels, radius, p, p, null)

    def apply(H=16, W=16, a=p, B=2, V=3):
        return lib.hrn_mncc_apply(a, p, p, B, V, H, W, p, p, null)

    for f in (grid, search, apply):
        assert f(a=null) == -2 and b"null" in lib.hrn_last_error()
        for bad in (dict(H=8), dict(H=129), dict(W=15), dict(W=129)):
            assert f(**bad) == -2 and b"shape" in lib.hrn_last_error(), bad
        assert f(B=0) == -2 and f(V=0) == -2 and b"batch" in lib.hrn_last_error()
    for f in (grid, search):
        assert f(P=2) == -2 and b"P=2" in lib.hrn_last_error()
        assert f(P=10) == -2 and b"P=10" in lib.hrn_last_error()
    assert search(levels=0) == -2 and b"levels" in lib.hrn_last_error()
    assert search(levels=17) == -2
    assert search(radius=0.0) == -2 and b"radius" in lib.hrn_last_error()
    assert search(radius=4.5) == -2 and search(radius=-1.0) == -2 and search(radius=float("nan")) == -2
    assert grid(width=0.0) == -2 and b"width" in lib.hrn_last_error()
    assert grid(width=8.5) == -2 and grid(width=float("nan")) == -2
    assert lib.hrn_mncc_search(p, p, p, p, 2, 3, 16, 16, 7, 6, 1.0, null, p, null) == -2 and b"null" in lib.hrn_last_error()
    assert lib.hrn_mncc_apply(p, p, p, 2, 3, 16, 16, p, null, null) == -2 and b"null" in lib.hrn_last_error()


def test_python_argument_errors():
    from hrnet_hip import registration as G
    a, m = torch.zeros(2, 3, 16, 20), torch.ones(2, 3, 16, 20)
    with pytest.raises(TypeError, match="torch.Tensor"):
        G.mncc_search(a.numpy())
    with pytest.raises(ValueError, match=r"\(B,V,H,W\).*\(2, 16, 20\)"):
        G.mncc_search(a[:, 0])
    with pytest.raises(ValueError, match=r"lr_masks.*\(2, 3, 16, 20\).*\(2, 3, 16, 16\)"):
        G.mncc_search(a, m[..., :16])
    with pytest.raises(ValueError, match=r"16\.\.128.*\(8, 20\)"):
        G.mncc_search(a[:, :, :8])
    with pytest.raises(ValueError, match=r"16\.\.128.*\(16, 129\)"):
        G.shift_views(torch.zeros(1, 2, 16, 129), None, torch.zeros(1, 2, 2))
    with pytest.raises(ValueError, match=r"ref must be \(B,H,W\) = \(2, 16, 20\).*\(2, 16, 16\)"):
        G.mncc_search(a, ref=a[:, 0, :, :16])
    with pytest.raises(ValueError, match="ref_mask"):
        G.mncc_search(a, ref_mask=m[:, 0])
    with pytest.raises(ValueError, match=r"ref_mask.*\(2, 16, 20\).*\(2, 3, 16, 20\)"):
        G.mncc_search(a, ref=a[:, 0], ref_mask=m)
    for bad, what in ((dict(points_per_dim=2), "points_per_dim"), (dict(points_per_dim=10), "points_per_dim"), (dict(levels=0), "levels"),
                      (dict(levels=17), "levels"), (dict(radius=0.0), "radius"), (dict(radius=4.1), "radius")):
        with pytest.raises(ValueError, match=what):
            G.mncc_search(a, m, **bad)
        with pytest.raises(ValueError, match=what):
            G.register_views(a, m, **bad)
    with pytest.raises(ValueError, match="width"):
        G.mncc_grid(a, m, width=0.0)
    with pytest.raises(ValueError, match=r"centres.*\(2, 3, 2\).*\(2, 3\)"):
        G.mncc_grid(a, m, centres=torch.zeros(2, 3))
    with pytest.raises(ValueError, match=r"shifts.*\(2, 3, 2\).*\(2, 2\)"):
        G.shift_views(a, m, torch.zeros(2, 2))
    with pytest.raises(TypeError, match="trace"):
        G.register_views(a, m, return_trace=True)
    for call in (lambda: G.mncc_search(a, m), lambda: G.mncc_grid(a, m), lambda: G.shift_views(a, m, torch.zeros(2, 3, 2)),
                 lambda: G.register_views(a)):
        with pytest.raises(TypeError, match="no CPU fallback"):
            call()


def test_fake_kernels_give_the_shapes():
    ops = torch.ops.hrnet_hip
    B, V, H, W = 2, 5, 24, 40
    views, masks = torch.empty(B, V, H, W, device="meta"), torch.empty(B, V, H, W, device="meta")
    ref = torch.empty(B, H, W, device="meta")
    scores = ops.mncc_grid(ref, None, views, masks, torch.empty(B, V, 2, device="meta"), 5, 0.5)
    assert scores.shape == (B, V, 5, 5) and scores.dtype == torch.float32 and scores.device.type == "meta"
    shifts, trace = ops.mncc_search(ref, ref, views, None, 7, 4, 1.0)
    assert shifts.shape == (B, V, 2) and trace.shape == (B, V, 4, 3) and shifts.dtype == trace.dtype == torch.float32
    out, valid = ops.shift_views(views.double(), masks, shifts)
    assert out.shape == valid.shape == (B, V, H, W) and out.dtype == valid.dtype == torch.float32


# ----------------------------------------------------------------------------- tools/registration_bench.py
def test_bench_tool_command_line():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import registration_bench as T
    assert vars(T.PARSER.parse_args([])) == dict(B=32, views=32, sizes=[128], points=7, levels=6, rounds=7, reps=5)
    got = vars(T.PARSER.parse_args("4 --views 8 --sizes 64,128 --points 5 --levels 4 --rounds 3 --reps 2".split()))
    assert got == dict(B=4, views=8, sizes=[64, 128], points=5, levels=4, rounds=3, reps=2)
    assert T.level_flops_per_pixel(7) == 7 * 12 + 49 * 32
    with pytest.raises(SystemExit) as e:
        T.PARSER.parse_args(["--bogus", "1"])
    assert e.value.code == 2


@pytest.mark.skipif(torch.cuda.is_available(), reason="there is a device: the tool would start measuring")
def test_bench_tool_refuses_to_run_without_a_device():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "registration_bench.py")], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 2 and "Traceback" not in r.stderr and r.stdout == ""
    assert r.stderr.strip().splitlines()[-1] == "registration_bench needs a ROCm device: a time cannot be measured without one"
