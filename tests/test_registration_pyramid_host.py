"""CPU: the host side of the coarse-to-fine registration search: the fp64 restatement
(tests/registration_pyramid_ref.py) - reduce2 keeps a constant, applies the mask rule at borders and under holes, takes odd sides, halves a
shift; the pyramid recovers shifts of up to 26 px that the plain search misses - the refusals of the C entry points before any launch,
the workspace formula, the fake kernels, and the argument errors of hrnet_hip.registration's functions.  Nothing here needs a GPU."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import registration_pyramid_ref as Y
import registration_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hrn_mncc_reduce2", "hrn_mncc_search_scene_from", "hrn_mncc_pyramid_workspace_bytes", "hrn_mncc_search_pyramid")

# (H, W), octaves, the limit of the true shifts in px: four views per seed, seeds 1..3, P = 7, the defaults of mncc_search_pyramid
ROWS = [((64, 80), 1, 7.0), ((96, 144), 2, 13.0), ((130, 203), 2, 14.0), ((160, 256), 3, 26.0)]
# The restatement's own worst error per row over the 12 views (the larger component of |found - true|), as this test measures it:
#   64 x 80: 0.00540 px    96 x 144: 0.00406 px    130 x 203: 0.00363 px    160 x 256: 0.00376 px
# No view is lost.  The device test of the first two rows bounds its error by 1.5 times these.
RESTATEMENT_WORST_PX = {(64, 80): 0.00540, (96, 144): 0.00406, (130, 203): 0.00363, (160, 256): 0.00376}
SHIFT_BOUND_PX = 0.02        # the project's bound on a recovered shift (sections 7f / 7g)
# How far the plain search gets from (0, 0) along an axis with P = 7, six levels and radius 4: every level may step to the edge of its
# grid, half a width, and the widths shrink by 1 / 4: 4 (1 + 1/4 + .. + 1/4^5) = 5.33203125 px, not 4.  A view within that is found; a view
# beyond it is missed by at least the excess, and by more than a pixel once a component passes 6.332 px.
PLAIN_REACH_PX = 4.0 * sum(0.25 ** k for k in range(6))


@pytest.fixture(scope="module")
def lib():
    from hrnet_hip import binding, build
    if not os.path.exists(binding.LIB_PATH):
        build.build_library(verbose=False)
    return binding.load_library()


# ----------------------------------------------------------------------------- reduce2
def test_reduce2_of_a_constant_is_that_constant_where_clear():
    rng = np.random.default_rng(5)
    for H, W in ((32, 32), (33, 47), (70, 96)):
        mask = (rng.random((H, W)) > 0.3).astype(np.float32)
        for m in (None, mask):
            v, clear, den = Y.reduce2(np.full((H, W), 0.37), m)
            assert v.shape == clear.shape == (H // 2, W // 2)
            assert np.abs(v[clear] - 0.37).max() < 1e-15 and np.all(v[~clear] == 0.0)
            assert clear.any() and (m is None or not clear.all())
        assert Y.reduce2(np.full((H, W), 0.37), None)[1].all()


def test_reduce2_mask_rule_at_borders_and_under_holes():
    H, W = 32, 40
    x = np.arange(H * W, dtype=np.float64).reshape(H, W) / (H * W)
    v, clear, den = Y.reduce2(x, None)
    # without a mask: the first row and column lose the taps outside the frame (weight 1/8 of the axis), the last of an even side too
    assert den[0, 0] == (7 / 8) ** 2 and den[0, 5] == 7 / 8 and den[5, 0] == 7 / 8 and den[5, 5] == 1.0
    assert den[-1, -1] == (7 / 8) ** 2 and den[-1, 5] == 7 / 8
    assert clear.all()
    # an interior pixel is the weighted mean of its 4 x 4 taps
    w = np.outer(Y.WEIGHTS, Y.WEIGHTS)
    assert abs(v[5, 7] - (w * x[9:13, 13:17]).sum()) < 1e-15
    # den is a multiple of 1/64 everywhere: exact in fp32
    assert np.all(den * 64 == np.round(den * 64))
    # a hole: the coarse pixel is clear iff more than half of its weight lies on clear pixels, and its value ignores what lies under the hole
    m = np.ones((H, W), np.float32)
    m[10:12, 14:16] = 0                                  # the four central taps of coarse pixel (5, 7): weight 36/64
    y = x.copy()
    y[10:12, 14:16] = np.nan
    v, clear, den = Y.reduce2(y, m)
    assert den[5, 7] == 28 / 64 and not clear[5, 7] and v[5, 7] == 0.0
    assert den[4, 7] == 1 - 6 / 64 and clear[4, 7] and np.isfinite(v).all()
    m[10:12, 14:16] = 1
    m[9, 13:17] = 0                                      # one outer row of taps: weight 1/8
    m[10, 13] = 0                                        # and 3/64 more: 1 - 8/64 - 3/64
    v, clear, den = Y.reduce2(x, m)
    assert den[5, 7] == 53 / 64 and clear[5, 7]
    keep = w * (m[9:13, 13:17] != 0)
    assert abs(v[5, 7] - (keep * x[9:13, 13:17]).sum() / keep.sum()) < 1e-15
    # exactly half is not clear: the threshold is strict
    m = np.ones((H, W), np.float32)
    m[9:13, 13:15] = 0
    assert Y.reduce2(x, m)[2][5, 7] == 0.5 and not Y.reduce2(x, m)[1][5, 7]


def test_reduce2_takes_odd_sides():
    x = np.random.default_rng(2).random((33, 47))
    v, clear, den = Y.reduce2(x, None)
    assert v.shape == (16, 23)
    # an odd side's last fine row / column is inside the frame: the last coarse pixel has all of its taps
    assert den[-1, -1] == 1.0 and den[-1, 0] == 7 / 8 and den[0, -1] == 7 / 8
    w = np.outer(Y.WEIGHTS, Y.WEIGHTS)
    assert abs(v[15, 22] - (w * x[29:33, 43:47]).sum()) < 1e-15


def test_a_fine_shift_is_half_a_coarse_shift():
    """The filter is even and symmetric and both sides are reduced alike: registering the reduced frames finds d / 2, with no offset.
    [1, 3, 3, 1] / 8 does not remove everything above the coarse Nyquist rate (these scenes keep about a tenth of their amplitude there), so
    the reduced view is not exactly the shifted reduced reference and d / 2 is met only roughly.  What the pyramid needs is that twice
    the coarse error stays inside the next octave's first grid, refine_radius = 1 px: 0.5 coarse px, which is the bound here."""
    true = np.array([[6.4, -3.0], [-5.0, 2.6]])
    ref, rm, views, vms = Y.scene(64, 80, true, seed=4)
    r1, rm1 = Y.octaves_of(ref, rm, 1)[1]
    for v in range(2):
        v1, vm1 = Y.octaves_of(views[v], vms[v], 1)[1]
        found, _ = R.search(r1, rm1, v1, vm1, P=7, levels=5, radius=4.0)
        assert np.abs(found - true[v] / 2).max() < 0.5, (found, true[v] / 2)


# ----------------------------------------------------------------------------- the pyramid
@functools.lru_cache(maxsize=None)
def recovered(shape, K, limit, seed):
    """-> (true (4, 2), pyramid's shifts (4, 2), plain search's shifts (4, 2)) for one seed of one row"""
    true = R.random_shifts(4, limit, seed=seed)
    ref, rm, views, vms = Y.scene(shape[0], shape[1], true, seed)
    got = np.stack([Y.pyramid(ref, rm, views[v], vms[v], octaves=K)[0] for v in range(4)])
    plain = np.stack([R.search(ref, rm, views[v], vms[v], P=7, levels=6, radius=4.0)[0] for v in range(4)])
    return true, got, plain


@pytest.mark.parametrize("shape,K,limit", ROWS, ids=["x".join(map(str, r[0])) for r in ROWS])
def test_restatement_recovers_shifts_beyond_the_search_radius(shape, K, limit):
    worst, far, gone = 0.0, 0, 0
    for seed in (1, 2, 3):
        true, got, plain = recovered(shape, K, limit, seed)
        err = np.abs(got - true).max(axis=1)
        worst = max(worst, float(err.max()))
        assert err.max() <= SHIFT_BOUND_PX, f"seed {seed}: a view is lost: errors {err}"
        # the control: the plain search with its largest radius cannot leave its reach, so it misses every view beyond it by the excess
        # at least, and by more than a pixel where a component of the true shift passes reach + 1
        size, plain_err = np.abs(true).max(axis=1), np.abs(plain - true).max(axis=1)
        beyond, lost = size > PLAIN_REACH_PX, size > PLAIN_REACH_PX + 1.0
        far, gone = far + int(beyond.sum()), gone + int(lost.sum())
        assert np.all(np.abs(plain) <= PLAIN_REACH_PX)
        assert np.all(plain_err[beyond] >= (size - PLAIN_REACH_PX)[beyond] - 1e-6) and np.all(plain_err[lost] > 1.0), (seed, plain, true)
        assert np.all(err[beyond] <= SHIFT_BOUND_PX)
    print(f"pyramid restatement {shape} K={K} +-{limit:g} px: worst error {worst:.5f} px over 12 views; the plain search misses {far} of "
          f"them, {gone} by more than a pixel")
    assert far >= 3
    assert abs(worst - RESTATEMENT_WORST_PX[shape]) < 5e-5, "the recorded figure is not what this test measures"


def test_pyramid_without_octaves_is_the_search():
    true = R.random_shifts(2, 0.9, seed=3)
    ref, rm, views, vms = R.scene(48, 40, true, seed=3)
    for v in range(2):
        s0, t0 = R.search(ref, rm, views[v], vms[v], P=5, levels=4, radius=1.0)
        s1, t1 = Y.pyramid(ref, rm, views[v], vms[v], octaves=0, P=5, levels=4, radius=1.0)
        assert np.array_equal(s0, s1) and np.array_equal(t0[-1], t1[0])
        s2, t2 = Y.search_from(ref, rm, views[v], vms[v], (0.0, 0.0), P=5, levels=4, radius=1.0)
        assert np.array_equal(s0, s2) and np.array_equal(t0, t2)


# ----------------------------------------------------------------------------- the C entry points
def test_exports_are_present(lib):
    from hrnet_hip import binding, build, registration
    header = open(os.path.join(ROOT, "include", "hrnet_hip.h")).read()
    for n in NAMES:
        assert n in binding.SIGNATURES and hasattr(lib, n) and n + "(" in header, n
    assert "registration_pyramid.hip" in build.SOURCES
    for f in ("reduce2", "mncc_search_pyramid", "register_scene_pyramid"):
        assert callable(getattr(registration, f)), f
    for op in ("reduce2", "mncc_search_scene_from", "mncc_search_pyramid"):
        assert hasattr(torch.ops.hrnet_hip, op), op


def _calls(lib):
    """The three entry points with good defaults; p is never dereferenced: every call made with these fails its checks first."""
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(64)

    def reduce(N=3, H=130, W=203, a=p, out=p):
        return lib.hrn_mncc_reduce2(a, p, N, H, W, out, p, null)

    def search_from(H=130, W=203, P=7, levels=4, radius=1.0, a=p, B=2, V=3, ws=p, shifts=p, short=0):
        return lib.hrn_mncc_search_scene_from(a, p, p, p, p, B, V, H, W, P, levels, radius, shifts, p, ws,
                                              max(lib.hrn_mncc_scene_workspace_bytes(B, V, H, W, P), 1) - short, null)

    def pyramid(H=130, W=203, P=7, octaves=2, levels=6, radius=4.0, coarse_levels=3, refine_radius=1.0, a=p, B=2, V=3, ws=p, shifts=p, short=0):
        return lib.hrn_mncc_search_pyramid(a, p, p, p, B, V, H, W, P, octaves, levels, radius, coarse_levels, refine_radius, shifts, p, ws,
                                           max(lib.hrn_mncc_pyramid_workspace_bytes(B, V, H, W, P, octaves), 1) - short, null)

    return null, reduce, search_from, pyramid


def test_c_entry_points_refuse_bad_arguments_before_any_launch(lib):
    null, reduce, search_from, pyramid = _calls(lib)
    err = lib.hrn_last_error
    assert reduce(a=null) == -2 and b"null" in err() and reduce(out=null) == -2 and b"null" in err()
    assert reduce(N=0) == -2 and b"N=0" in err()
    for bad in (dict(H=31), dict(W=31), dict(H=16385), dict(W=16385)):
        assert reduce(**bad) == -2 and b"shape" in err() and b"32..16384" in err(), bad
    assert reduce(N=1 << 17, H=16384, W=16384) == -2 and b"exceed one launch" in err()
    for f in (search_from, pyramid):
        assert f(a=null) == -2 and b"null" in err()
        assert f(ws=null) == -2 and b"null" in err() and f(shifts=null) == -2 and b"null" in err()
        for bad in (dict(H=15), dict(W=15), dict(H=16385), dict(W=16385)):
            assert f(**bad) == -2 and b"shape" in err(), bad
        assert f(B=0) == -2 and f(V=0) == -2 and b"batch" in err()
        assert f(B=1 << 15, V=1, H=16384, W=16384) == -2 and b"exceed one launch" in err()
        assert f(P=2) == -2 and b"P=2" in err() and f(P=10) == -2 and b"P=10" in err()
        assert f(levels=0) == -2 and b"levels" in err() and f(levels=17) == -2
        assert f(radius=0.0) == -2 and b"radius" in err() and f(radius=4.5) == -2 and f(radius=float("nan")) == -2
    assert pyramid(octaves=-1) == -2 and b"octaves" in err() and pyramid(octaves=7) == -2 and b"octaves" in err()
    assert pyramid(coarse_levels=0) == -2 and b"coarse_levels" in err() and pyramid(coarse_levels=17) == -2
    assert pyramid(refine_radius=0.0) == -2 and b"refine_radius" in err() and pyramid(refine_radius=4.5) == -2
    assert pyramid(refine_radius=float("nan")) == -2
    assert pyramid(H=2048, W=2048, octaves=6, radius=4.0) == -2 and b"reaches" in err()          # 256 px
    assert pyramid(H=2048, W=2048, octaves=6, radius=2.5) == -2 and b"reaches" in err()          # 160 px
    assert pyramid(H=130, W=63, octaves=2) == -2 and b"octave 2" in err()                        # 63 >> 2 = 15
    assert pyramid(H=31, W=203, octaves=1) == -2 and b"octave 1" in err()


def test_c_entry_points_refuse_a_workspace_one_byte_short(lib):
    _, _, search_from, pyramid = _calls(lib)
    for shape in (dict(), dict(H=16, W=16), dict(B=1, V=1, H=257, W=144, P=9)):
        assert search_from(short=1, **shape) == -3 and b"workspace" in lib.hrn_last_error(), shape
    for shape in (dict(), dict(H=16, W=16, octaves=0), dict(B=1, V=1, H=257, W=144, P=9, octaves=3), dict(H=2048, W=1536, octaves=5)):
        assert pyramid(short=1, **shape) == -3 and b"workspace" in lib.hrn_last_error(), shape


def test_workspace_size(lib):
    need = lib.hrn_mncc_pyramid_workspace_bytes
    for bad in ((0, 1, 64, 64, 7, 1), (1, 0, 64, 64, 7, 1), (1, 1, 15, 64, 7, 0), (1, 1, 64, 16385, 7, 1), (1, 1, 64, 64, 2, 1),
                (1, 1, 64, 64, 10, 1), (1, 1, 64, 64, 7, -1), (1, 1, 64, 64, 7, 7), (1, 1, 64, 64, 7, 3), (1, 1, 130, 63, 7, 2),
                (1 << 15, 1, 16384, 16384, 7, 1)):
        assert need(*bad) == 0, bad

    def r16(n):
        return -(-n // 16) * 16

    for B, V, H, W, P, K in ((1, 2, 16, 16, 7, 0), (1, 2, 64, 80, 7, 1), (1, 2, 130, 203, 7, 2), (2, 3, 257, 145, 9, 3), (1, 1, 33, 47, 3, 1),
                             (2, 32, 512, 512, 7, 3), (1, 32, 8192, 6144, 9, 6)):
        planes = sum(r16(8 * (B * V + B) * (H >> k) * (W >> k)) for k in range(1, K + 1))
        assert need(B, V, H, W, P, K) == planes + r16(lib.hrn_mncc_scene_workspace_bytes(B, V, H, W, P)) + 16 * B * V, (B, V, H, W, P, K)


# ----------------------------------------------------------------------------- ops and Python arguments
def test_fake_kernels_give_the_shapes():
    ops = torch.ops.hrnet_hip
    B, V, H, W = 2, 5, 130, 203
    views, masks = torch.empty(B, V, H, W, device="meta"), torch.empty(B, V, H, W, device="meta")
    ref, init = torch.empty(B, H, W, device="meta"), torch.empty(B, V, 2, device="meta")
    out, om = ops.reduce2(views.reshape(-1, H, W), None)
    assert out.shape == om.shape == (B * V, 65, 101) and out.dtype == om.dtype == torch.float32 and out.device.type == "meta"
    out, om = ops.reduce2(ref.double(), ref)
    assert out.shape == om.shape == (B, 65, 101) and out.dtype == torch.float32
    shifts, trace = ops.mncc_search_scene_from(ref, None, views, masks, init, 7, 4, 1.0)
    assert shifts.shape == (B, V, 2) and trace.shape == (B, V, 4, 3) and shifts.dtype == trace.dtype == torch.float32
    shifts, trace = ops.mncc_search_scene_from(ref, ref, views, None, None, 5, 2, 4.0)
    assert shifts.shape == (B, V, 2) and trace.shape == (B, V, 2, 3)
    shifts, trace = ops.mncc_search_pyramid(ref, ref, views, masks, 2, 7, 6, 4.0, 3, 1.0)
    assert shifts.shape == (B, V, 2) and trace.shape == (B, V, 3, 3) and shifts.dtype == trace.dtype == torch.float32
    assert ops.mncc_search_pyramid(ref, None, views, None, 0, 7, 6, 4.0, 3, 1.0)[1].shape == (B, V, 1, 3)


def test_python_argument_errors():
    from hrnet_hip import registration as G
    a, m = torch.zeros(2, 3, 130, 203), torch.ones(2, 3, 130, 203)
    with pytest.raises(TypeError, match="torch.Tensor"):
        G.reduce2(a.numpy())
    with pytest.raises(ValueError, match=r"\(B,V,H,W\) or \(B,H,W\).*\(130, 203\)"):
        G.reduce2(a[0, 0])
    with pytest.raises(TypeError, match="masks must be a torch.Tensor"):
        G.reduce2(a, m.numpy())
    with pytest.raises(ValueError, match=r"masks.*\(2, 3, 130, 203\).*\(2, 130, 203\)"):
        G.reduce2(a, m[:, 0])
    with pytest.raises(ValueError, match=r"32\.\.16384.*\(31, 40\)"):
        G.reduce2(torch.zeros(1, 31, 40))
    with pytest.raises(ValueError, match=r"32\.\.16384.*\(32, 16385\)"):
        G.reduce2(torch.zeros(1, 1, 32, 16385))
    with pytest.raises(TypeError, match="init must be a torch.Tensor"):
        G.mncc_search_scene(a, m, init=np.zeros((2, 3, 2)))
    with pytest.raises(ValueError, match=r"init.*\(2, 3, 2\).*\(2, 3\)"):
        G.mncc_search_scene(a, m, init=torch.zeros(2, 3))
    with pytest.raises(TypeError, match="torch.Tensor"):
        G.mncc_search_pyramid(a.numpy())
    with pytest.raises(ValueError, match=r"\(B,V,H,W\).*\(2, 130, 203\)"):
        G.mncc_search_pyramid(a[:, 0])
    with pytest.raises(ValueError, match=r"ref must be \(B,H,W\) = \(2, 130, 203\)"):
        G.mncc_search_pyramid(a, ref=a[:, 0, :, :16])
    for bad, what in ((dict(points_per_dim=2), "points_per_dim"), (dict(points_per_dim=10), "points_per_dim"), (dict(levels=0), "levels"),
                      (dict(levels=17), "levels"), (dict(radius=0.0), "radius"), (dict(radius=4.1), "radius"), (dict(octaves=-1), "octaves"),
                      (dict(octaves=7), "octaves"), (dict(coarse_levels=0), "coarse_levels"), (dict(coarse_levels=17), "coarse_levels"),
                      (dict(refine_radius=0.0), "refine_radius"), (dict(refine_radius=4.1), "refine_radius"),
                      (dict(octaves=4), r"octave 4.*at least 16.*\(130, 203\)")):
        for f in (G.mncc_search_pyramid, G.register_scene_pyramid):
            with pytest.raises(ValueError, match=what):
                f(a, m, **bad)
    big = torch.zeros(1, 1, 1, 1).expand(1, 2, 2048, 2048)
    with pytest.raises(ValueError, match=r"radius \* 2\*\*octaves.*128"):
        G.mncc_search_pyramid(big, octaves=6, radius=4.0)
    with pytest.raises(ValueError, match="octaves"):
        G.register_scene_local(a, m, octaves=7)
    with pytest.raises(TypeError, match="trace"):
        G.register_scene_pyramid(a, m, return_trace=True)
    for call in (lambda: G.reduce2(a), lambda: G.reduce2(a[:, 0], m[:, 0]), lambda: G.mncc_search_scene(a, m, init=torch.zeros(2, 3, 2)),
                 lambda: G.mncc_search_pyramid(a, m), lambda: G.register_scene_pyramid(a), lambda: G.register_scene_local(a, m, octaves=2)):
        with pytest.raises(TypeError, match="no CPU fallback"):
            call()


# ----------------------------------------------------------------------------- tools/registration_pyramid_bench.py
def test_bench_tool_command_line():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import registration_pyramid_bench as T
    assert "import _common" in open(T.__file__).read()
    assert vars(T.PARSER.parse_args([])) == dict(B=2, views=32, size=512, octaves=3, points=7, levels=6, coarse_levels=3, rounds=7, reps=5)
    got = vars(T.PARSER.parse_args("1 --views 4 --size 200 --octaves 2 --points 5 --levels 4 --coarse-levels 2 --rounds 3 --reps 2".split()))
    assert got == dict(B=1, views=4, size=200, octaves=2, points=5, levels=4, coarse_levels=2, rounds=3, reps=2)
    with pytest.raises(SystemExit) as e:
        T.PARSER.parse_args(["--bogus", "1"])
    assert e.value.code == 2


@pytest.mark.skipif(torch.cuda.is_available(), reason="there is a device: the tool would start measuring")
def test_bench_tool_refuses_to_run_without_a_device():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "registration_pyramid_bench.py")], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 2 and "Traceback" not in r.stderr and r.stdout == ""
    assert r.stderr.strip().splitlines()[-1] == "registration_pyramid_bench needs a ROCm device: a time cannot be measured without one"
