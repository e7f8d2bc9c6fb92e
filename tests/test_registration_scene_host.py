"""CPU: the host side of the masked-NCC registration for frames of any size.  The exports, the refusals of the C
entry points before any launch, the workspace size, the fake kernels, the argument errors of hrnet_hip.registration's *_scene functions,
tools/registration_scene_bench.py's command line, and that the fp64 restatement (tests/registration_ref.py, which has no size limit)
recovers known shifts on frames beyond 128 pixels a side.  Nothing here needs a GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import registration_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECOVERY_PX = 0.02           # the project's bound on every component of a recovered shift
NAMES = ("hrn_mncc_scene_workspace_bytes", "hrn_mncc_grid_scene", "hrn_mncc_search_scene", "hrn_mncc_apply_scene")


@pytest.fixture(scope="module")
def lib():
    from hrnet_hip import binding, build
    if not os.path.exists(binding.LIB_PATH):
        build.build_library(verbose=False)
    return binding.load_library()


# ----------------------------------------------------------------------------- the restatement on large frames
# (H, W, limit of the true shifts, radius, levels): measured on the CPU at P = 7, three views each: worst error 0.0031, 0.0035, 0.0042,
# 0.0034 and 0.0027 px
LARGE = [(130, 203, 0.9, 1.0, 5), (257, 144, 0.9, 1.0, 5), (16, 300, 0.9, 1.0, 5), (200, 136, 3.5, 4.0, 7), (130, 203, 1.8, 2.0, 6)]


@pytest.mark.parametrize("H,W,limit,radius,levels", LARGE, ids=[f"{h}x{w}_r{int(r)}" for h, w, _, r, _ in LARGE])
def test_restatement_recovers_known_shifts_beyond_128(H, W, limit, radius, levels):
    shifts = R.random_shifts(3, limit, seed=7000 + H * W)
    ref, ref_mask, views, view_masks = R.scene(H, W, shifts, seed=H * W)
    for v in range(3):
        got, trace = R.search(ref, ref_mask, views[v], view_masks[v], 7, levels, radius)
        err = np.abs(got.astype(np.float64) - shifts[v])
        print(f"{H}x{W} radius {radius} view {v}: true {shifts[v]}, found {got}, error {err.max():.4f} px, score {trace[-1, 2]:.6f}")
        assert err.max() <= RECOVERY_PX


# ----------------------------------------------------------------------------- the new surface
def test_exports_are_present(lib):
    import hrnet_hip
    from hrnet_hip import binding, build, registration
    header = open(os.path.join(ROOT, "include", "hrnet_hip.h")).read()
    for n in NAMES:
        assert n in binding.SIGNATURES and hasattr(lib, n) and n + "(" in header, n
    assert "registration_scene.hip" in build.SOURCES and "registration.hip" in build.SOURCES
    assert os.path.exists(os.path.join(os.path.dirname(build.__file__), "csrc", "registration_scene.hip"))
    assert hrnet_hip.registration is registration


def test_python_functions_and_ops_exist():
    from hrnet_hip import binding, registration
    for f in ("mncc_search_scene", "mncc_grid_scene", "shift_scene", "register_scene"):
        assert callable(getattr(registration, f)), f
    for f in ("mncc_grid_scene", "mncc_search_scene", "mncc_apply_scene"):
        assert callable(getattr(binding, f)), f
    for op in ("mncc_grid_scene", "mncc_search_scene", "shift_scene"):
        assert hasattr(torch.ops.hrnet_hip, op), op


def _calls(lib):
    """The three entry points with good defaults; p is never dereferenced: every call made with these fails its checks first."""
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(64)

    def need(B=2, V=3, H=16, W=16, P=7):
        return lib.hrn_mncc_scene_workspace_bytes(B, V, H, W, P)

    def grid(H=16, W=16, P=7, width=2.0, a=p, B=2, V=3, ws=p, short=0):
        return lib.hrn_mncc_grid_scene(a, p, p, p, p, B, V, H, W, P, width, p, ws, max(need(B, V, H, W, P), 1) - short, null)

    def search(H=16, W=16, P=7, levels=6, radius=1.0, a=p, B=2, V=3, ws=p, short=0):
        return lib.hrn_mncc_search_scene(a, p, p, p, B, V, H, W, P, levels, radius, p, p, ws, max(need(B, V, H, W, P), 1) - short, null)

    def apply(H=16, W=16, a=p, B=2, V=3):
        return lib.hrn_mncc_apply_scene(a, p, p, B, V, H, W, p, p, null)

    return null, p, grid, search, apply


def test_c_entry_points_refuse_bad_arguments_before_any_launch(lib):
    null, p, grid, search, apply = _calls(lib)
    for f in (grid, search, apply):
        assert f(a=null) == -2 and b"null" in lib.hrn_last_error()
        for bad in (dict(H=15), dict(W=15), dict(H=16385), dict(W=16385)):
            assert f(**bad) == -2 and b"shape" in lib.hrn_last_error() and b"16..16384" in lib.hrn_last_error(), bad
        assert f(B=0) == -2 and f(V=0) == -2 and b"batch" in lib.hrn_last_error()
    for f in (grid, search):
        assert f(P=2) == -2 and b"P=2" in lib.hrn_last_error()
        assert f(P=10) == -2 and b"P=10" in lib.hrn_last_error()
        assert f(ws=null) == -2 and b"null" in lib.hrn_last_error()
    assert search(levels=0) == -2 and b"levels" in lib.hrn_last_error()
    assert search(levels=17) == -2
    assert search(radius=0.0) == -2 and b"radius" in lib.hrn_last_error()
    assert search(radius=4.5) == -2 and search(radius=-1.0) == -2 and search(radius=float("nan")) == -2
    assert grid(width=0.0) == -2 and b"width" in lib.hrn_last_error()
    assert grid(width=8.5) == -2 and grid(width=float("nan")) == -2
    assert lib.hrn_mncc_search_scene(p, p, p, p, 2, 3, 16, 16, 7, 6, 1.0, null, p, p, 1 << 30, null) == -2 and b"null" in lib.hrn_last_error()
    assert lib.hrn_mncc_apply_scene(p, p, p, 2, 3, 16, 16, p, null, null) == -2 and b"null" in lib.hrn_last_error()
    # a frame that the LDS-resident entry points refuse is refused here for another reason only
    assert grid(H=129, W=16384, a=null) == -2 and b"null" in lib.hrn_last_error()


def test_c_entry_points_refuse_a_workspace_one_byte_short(lib):
    _, _, grid, search, _ = _calls(lib)
    for f in (grid, search):
        for shape in (dict(), dict(H=130, W=203), dict(B=1, V=1, H=64, W=64, P=9)):
            assert f(short=1, **shape) == -3 and b"workspace" in lib.hrn_last_error(), shape


def test_workspace_size(lib):
    need = lib.hrn_mncc_scene_workspace_bytes
    for bad in ((0, 1, 64, 64, 7), (1, 0, 64, 64, 7), (1, 1, 15, 64, 7), (1, 1, 64, 16385, 7), (1, 1, 64, 64, 2), (1, 1, 64, 64, 10), (-1, 1, 64, 64, 7)):
        assert need(*bad) == 0, bad
    # the formula of include/hrnet_hip.h
    for B, V, H, W, P in ((1, 1, 64, 64, 9), (2, 3, 130, 203, 7), (32, 32, 512, 512, 9), (1, 32, 8192, 6144, 9), (3, 2, 16, 300, 3)):
        T, C = -(-H // 64) * -(-W // 64), min(64, -(-H * W // 16384))
        assert need(B, V, H, W, P) == 16 * (B * V + B) * C + 48 * P * P * B * V * T + 8 * B * V, (B, V, H, W, P)
    # monotone in each argument
    base = dict(B=2, V=3, H=100, W=150, P=5)
    for name, values in (("B", (1, 2, 3, 40)), ("V", (1, 2, 3, 40)), ("H", (16, 64, 65, 128, 129, 1000, 16384)),
                         ("W", (16, 64, 65, 128, 129, 1000, 16384)), ("P", range(3, 10))):
        sizes = [need(*dict(base, **{name: v}).values()) for v in values]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes), (name, sizes)
    # at most the bytes of `views`
    for B, V, H, W, P in ((1, 1, 64, 64, 9), (32, 32, 512, 512, 9), (1, 32, 8192, 6144, 9), (1, 1, 65, 65, 9), (4, 1, 65, 64, 9)):
        assert 0 < need(B, V, H, W, P) <= 4 * B * V * H * W, (B, V, H, W, P)


def test_fake_kernels_give_the_shapes():
    ops = torch.ops.hrnet_hip
    B, V, H, W = 2, 5, 200, 136
    views, masks = torch.empty(B, V, H, W, device="meta"), torch.empty(B, V, H, W, device="meta")
    ref = torch.empty(B, H, W, device="meta")
    scores = ops.mncc_grid_scene(ref, None, views, masks, torch.empty(B, V, 2, device="meta"), 5, 0.5)
    assert scores.shape == (B, V, 5, 5) and scores.dtype == torch.float32 and scores.device.type == "meta"
    shifts, trace = ops.mncc_search_scene(ref, ref, views, None, 7, 4, 1.0)
    assert shifts.shape == (B, V, 2) and trace.shape == (B, V, 4, 3) and shifts.dtype == trace.dtype == torch.float32
    out, valid = ops.shift_scene(views.double(), masks, shifts)
    assert out.shape == valid.shape == (B, V, H, W) and out.dtype == valid.dtype == torch.float32


def test_python_argument_errors():
    from hrnet_hip import registration as G
    a, m = torch.zeros(2, 3, 200, 136), torch.ones(2, 3, 200, 136)
    with pytest.raises(TypeError, match="torch.Tensor"):
        G.mncc_search_scene(a.numpy())
    with pytest.raises(ValueError, match=r"\(B,V,H,W\).*\(2, 200, 136\)"):
        G.mncc_search_scene(a[:, 0])
    with pytest.raises(ValueError, match=r"lr_masks.*\(2, 3, 200, 136\).*\(2, 3, 200, 16\)"):
        G.mncc_search_scene(a, m[..., :16])
    with pytest.raises(ValueError, match=r"16\.\.16384.*\(8, 20\)"):
        G.mncc_search_scene(torch.zeros(1, 2, 8, 20))
    with pytest.raises(ValueError, match=r"16\.\.16384.*\(16, 16385\)"):
        G.shift_scene(torch.zeros(1, 1, 16, 16385), None, torch.zeros(1, 1, 2))
    with pytest.raises(ValueError, match=r"16\.\.16384.*\(8, 20\)"):
        G.mncc_grid_scene(torch.zeros(1, 2, 8, 20))
    with pytest.raises(ValueError, match=r"ref must be \(B,H,W\) = \(2, 200, 136\).*\(2, 200, 16\)"):
        G.mncc_search_scene(a, ref=a[:, 0, :, :16])
    with pytest.raises(ValueError, match="ref_mask"):
        G.mncc_search_scene(a, ref_mask=m[:, 0])
    for bad, what in ((dict(points_per_dim=2), "points_per_dim"), (dict(points_per_dim=10), "points_per_dim"), (dict(levels=0), "levels"),
                      (dict(levels=17), "levels"), (dict(radius=0.0), "radius"), (dict(radius=4.1), "radius")):
        with pytest.raises(ValueError, match=what):
            G.mncc_search_scene(a, m, **bad)
        with pytest.raises(ValueError, match=what):
            G.register_scene(a, m, **bad)
    with pytest.raises(ValueError, match="width"):
        G.mncc_grid_scene(a, m, width=8.5)
    with pytest.raises(ValueError, match=r"centres.*\(2, 3, 2\).*\(2, 3\)"):
        G.mncc_grid_scene(a, m, centres=torch.zeros(2, 3))
    with pytest.raises(ValueError, match=r"shifts.*\(2, 3, 2\).*\(2, 2\)"):
        G.shift_scene(a, m, torch.zeros(2, 2))
    with pytest.raises(TypeError, match="trace"):
        G.register_scene(a, m, return_trace=True)
    for call in (lambda: G.mncc_search_scene(a, m), lambda: G.mncc_grid_scene(a, m), lambda: G.shift_scene(a, m, torch.zeros(2, 3, 2)),
                 lambda: G.register_scene(a)):
        with pytest.raises(TypeError, match="no CPU fallback"):
            call()


def test_the_lds_resident_functions_keep_their_limit():
    from hrnet_hip import registration as G
    with pytest.raises(ValueError, match=r"16\.\.128.*\(16, 129\)"):
        G.shift_views(torch.zeros(1, 2, 16, 129), None, torch.zeros(1, 2, 2))
    for call in (lambda: G.mncc_search(torch.zeros(1, 2, 129, 16)), lambda: G.mncc_grid(torch.zeros(1, 2, 16, 200)),
                 lambda: G.register_views(torch.zeros(1, 2, 130, 203))):
        with pytest.raises(ValueError, match=r"16\.\.128"):
            call()


# ----------------------------------------------------------------------------- tools/registration_scene_bench.py
def test_bench_tool_command_line():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import registration_scene_bench as T
    assert vars(T.PARSER.parse_args([])) == dict(B=2, views=32, size=512, lds_batch=32, lds_size=128, points=7, levels=6, rounds=7, reps=5)
    got = vars(T.PARSER.parse_args("1 --views 4 --size 200 --lds-batch 2 --lds-size 64 --points 5 --levels 4 --rounds 3 --reps 2".split()))
    assert got == dict(B=1, views=4, size=200, lds_batch=2, lds_size=64, points=5, levels=4, rounds=3, reps=2)
    with pytest.raises(SystemExit) as e:
        T.PARSER.parse_args(["--bogus", "1"])
    assert e.value.code == 2


@pytest.mark.skipif(torch.cuda.is_available(), reason="there is a device: the tool would start measuring")
def test_bench_tool_refuses_to_run_without_a_device():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "registration_scene_bench.py")], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 2 and "Traceback" not in r.stderr and r.stdout == ""
    assert r.stderr.strip().splitlines()[-1] == "registration_scene_bench needs a ROCm device: a time cannot be measured without one"
