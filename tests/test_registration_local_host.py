"""CPU: the host side of the shift field of a scene: the blocks of an axis as the library counts them, the fp64
restatement (tests/registration_local_ref.py) - one block is registration_ref.search, a known linear field is recovered at the nodes and
beats the one global shift between them, a block without enough common pixels falls back to `init` - the refusals of the C entry
points before any launch, the workspace formula, the fake kernels, the argument errors of hrnet_hip.registration's functions and
tools/registration_local_bench.py's command line.  Nothing here needs a GPU."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import registration_local_ref as L
import registration_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hrn_mncc_local_blocks", "hrn_mncc_local_workspace_bytes", "hrn_mncc_search_local", "hrn_mncc_apply_field")
# The restatement's own worst node error on the linear field at 130 x 203, block 64, P = 7, five global levels of radius 1 and four local
# ones of radius 0.5: 0.0190, 0.0194 and 0.0243 px for seeds 1, 2, 3 (the Euclidean distance to the fixed point at the node); times 1.5
# for the spread from seed to seed.  The device test of the same scene uses this bound.
NODE_BOUND_PX = 1.5 * 0.0243


@pytest.fixture(scope="module")
def lib():
    from hrnet_hip import binding, build
    if not os.path.exists(binding.LIB_PATH):
        build.build_library(verbose=False)
    return binding.load_library()


# ----------------------------------------------------------------------------- blocks
COUNTS = {(16, 64): 1, (96, 64): 2, (130, 64): 2, (257, 64): 4, (16384, 64): 256, (16, 128): 1, (96, 128): 1, (130, 128): 1, (257, 128): 2,
          (16384, 128): 128, (16, 4096): 1, (96, 4096): 1, (130, 4096): 1, (257, 4096): 1, (16384, 4096): 4}


def test_block_counts_and_bounds(lib):
    from hrnet_hip import registration as G
    for (length, block), n in COUNTS.items():
        assert lib.hrn_mncc_local_blocks(length, block) == n == L.blocks(length, block), (length, block)
        b = L.bounds(length, block)
        assert len(b) == n and b[0][0] == 0 and b[-1][1] == length and all(b[i][1] == b[i + 1][0] for i in range(n - 1))
        assert all(r0 % 64 == 0 and r1 - r0 == block for r0, r1 in b[:-1]) and (n == 1 or block / 2 <= b[-1][1] - b[-1][0] < 1.5 * block)
    assert L.bounds(130, 64) == [(0, 64), (64, 130)] and L.bounds(257, 128) == [(0, 128), (128, 257)] and L.bounds(96, 64) == [(0, 64), (64, 96)]
    assert L.bounds(191, 128) == [(0, 191)] and L.bounds(192, 128) == [(0, 128), (128, 192)]
    assert list(L.nodes(130, 64)) == [31.5, 96.5] and list(L.nodes(257, 128)) == [63.5, 192.0] and list(L.nodes(16, 64)) == [7.5]
    assert G.local_blocks(130, 203, 64) == (2, 3) and G.local_blocks(257, 144, 128) == (2, 1) and G.local_blocks(200, 264, 64) == (3, 4)
    for bad in (0, 32, 63, 96, 100, 4160, 8192, -64):
        assert lib.hrn_mncc_local_blocks(130, bad) == 0, bad
        with pytest.raises(ValueError, match="multiple of 64"):
            G.local_blocks(130, 203, bad)
    assert lib.hrn_mncc_local_blocks(0, 64) == 0 and lib.hrn_mncc_local_blocks(16385, 64) == 0


# ----------------------------------------------------------------------------- the restatement
def test_one_block_is_the_global_search():
    shifts = R.random_shifts(2, 0.9, seed=11)
    ref, ref_mask, views, view_masks = R.scene(70, 90, shifts, seed=12)
    for v, (rm, vm) in enumerate(((ref_mask, view_masks[0]), (None, None))):
        want, want_trace = R.search(ref, rm, views[v], vm, 7, 4, 1.0)
        field, trace, ok, n = L.search_local(ref, rm, views[v], vm, 4096, None, 7, 4, 1.0, 0.0)
        assert field.shape == (1, 1, 2) and np.array_equal(field[0, 0], want) and np.array_equal(trace[0, 0], want_trace) and ok.all()
        assert np.abs(want - shifts[v]).max() <= 0.02


@functools.lru_cache(maxsize=None)
def recovery(seed):
    H, W, block = 130, 203, 64
    t = L.linear_field(H, W)
    ref, ref_mask, views, view_masks = L.warped_scene(H, W, [t], seed)
    shift, _ = R.search(ref, ref_mask, views[0], view_masks[0], 7, 5, 1.0)
    field, _, ok, _ = L.search_local(ref, ref_mask, views[0], view_masks[0], block, shift, 7, 4, 0.5, 0.25)
    return t, shift, field, ok


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_restatement_recovers_a_linear_field(seed):
    H, W, block = 130, 203, 64
    t, shift, field, ok = recovery(seed)
    assert ok.all() and field.shape == (2, 3, 2)
    ny, nx = np.meshgrid(L.nodes(H, block), L.nodes(W, block), indexing="ij")
    node_err = np.sqrt(((field.astype(np.float64) - L.recovered(t, ny, nx)) ** 2).sum(-1))
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    truth = L.recovered(t, y, x)
    local = np.sqrt(((L.field_at_pixels(field, H, W, block).astype(np.float64) - truth) ** 2).sum(-1))
    glob = np.sqrt(((shift.astype(np.float64) - truth) ** 2).sum(-1))
    print(f"seed {seed}: global shift {shift}; node error {node_err.min():.4f} .. {node_err.max():.4f} px; per pixel: local mean "
          f"{local.mean():.4f} max {local.max():.4f}, global mean {glob.mean():.4f} max {glob.max():.4f} px")
    assert node_err.max() <= NODE_BOUND_PX
    assert local.mean() < glob.mean() / 3.0


def test_field_at_pixels_is_bilinear_between_nodes_and_constant_beyond():
    H, W, block = 130, 203, 64
    field = np.arange(12, dtype=np.float32).reshape(2, 3, 2) / 8
    f = L.field_at_pixels(field, H, W, block, rounded=False)
    assert np.array_equal(f[:32, :32], np.broadcast_to(field[0, 0], (32, 32, 2))) and np.array_equal(f[97:, 165:], np.broadcast_to(field[1, 2], (33, 38, 2)))
    assert np.allclose(f[64, 63], 0.5 * (0.5 * (field[0, 0] + field[0, 1]) + 0.5 * (field[1, 0] + field[1, 1])), atol=0.02)
    ky, _, ty = L.axis_weights(H, block)
    assert ky.max() == 0 and ty[31] == 0.0 and ty[32] == 0.5 / 65 and ty[96] == 64.5 / 65 and ty[97] == 1.0
    one = L.field_at_pixels(field[:1, :1], 16, 16, 64)
    assert np.array_equal(one, np.broadcast_to(field[0, 0], (16, 16, 2)))
    const = np.broadcast_to(np.float32([0.37, -1.62]), (2, 3, 2))
    assert np.array_equal(L.field_at_pixels(const, H, W, block), np.broadcast_to(const[0, 0], (H, W, 2)))


def test_sampler_by_a_constant_field_is_the_global_sampler():
    shifts = R.random_shifts(1, 0.9, seed=3)
    _, _, views, view_masks = R.scene(40, 50, shifts, seed=4)
    for s in ((0.37, -1.62), (-3.5, 2.25)):
        px = np.broadcast_to(np.float32(s), (40, 50, 2))
        out, valid, _ = L.sample_field(views[0], view_masks[0], px)
        want_valid = R.shifted_mask(view_masks[0], s)
        assert np.array_equal(valid, want_valid) and np.all(out[~valid] == 0.0)
        assert np.abs(out - R.sample(views[0], s))[valid].max() <= 1e-15


def test_blocks_without_enough_common_pixels_keep_init():
    ref, ref_mask, views, view_masks = L.fallback_cases()
    init = np.float32(L.FALLBACK_INIT)
    for v, finite in ((0, False), (1, True)):
        field, trace, ok, n = L.search_local(ref, ref_mask, views[v], view_masks[v], L.FALLBACK_BLOCK, init, 5, 3, 0.5, 0.25)
        print(f"view {v}: n {n.tolist()}, threshold {[0.25 * 70 * 64, 0.25 * 70 * 76]}, last scores {trace[0, :, -1, 2]}")
        assert ok.tolist() == [[False, True]]
        assert np.array_equal(field[0, 0], init) and np.isfinite(trace[0, 0, -1, 2]) == finite
        assert (n[0, 0] == 0) if not finite else (0 < n[0, 0] <= 441)
        assert np.abs(field[0, 1] - init).max() <= 0.02 and np.isfinite(trace[0, 1, -1, 2])
        for j, area in ((0, 70 * 64), (1, 70 * 76)):
            assert abs(n[0, j] - 0.25 * area) > 0.01 * 0.25 * area


# ----------------------------------------------------------------------------- the new surface
def test_exports_are_present(lib):
    from hrnet_hip import binding, build
    header = open(os.path.join(ROOT, "include", "hrnet_hip.h")).read()
    for n in NAMES:
        assert n in binding.SIGNATURES and hasattr(lib, n) and n + "(" in header, n
    assert "registration_local.hip" in build.SOURCES
    from hrnet_hip import registration
    for f in ("mncc_search_local", "shift_field", "register_scene_local", "local_blocks"):
        assert callable(getattr(registration, f)), f
    for op in ("mncc_search_local", "shift_field"):
        assert hasattr(torch.ops.hrnet_hip, op), op


def _calls(lib):
    """The two entry points with good defaults; p is never dereferenced: every call made with these fails its checks first."""
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(64)

    def need(B=2, V=3, H=130, W=203, P=7, block=64):
        return lib.hrn_mncc_local_workspace_bytes(B, V, H, W, P, block)

    def search(H=130, W=203, P=7, levels=4, radius=0.5, block=64, min_valid=0.25, a=p, B=2, V=3, ws=p, field=p, short=0):
        return lib.hrn_mncc_search_local(a, p, p, p, p, B, V, H, W, P, levels, radius, block, min_valid, field, p, p, ws,
                                         max(need(B, V, H, W, P, block), 1) - short, null)

    def apply(H=130, W=203, block=64, a=p, B=2, V=3, out=p):
        return lib.hrn_mncc_apply_field(a, p, p, B, V, H, W, block, out, p, null)

    return null, p, need, search, apply


def test_c_entry_points_refuse_bad_arguments_before_any_launch(lib):
    null, p, need, search, apply = _calls(lib)
    for f in (search, apply):
        assert f(a=null) == -2 and b"null" in lib.hrn_last_error()
        for bad in (dict(H=15), dict(W=15), dict(H=16385), dict(W=16385)):
            assert f(**bad) == -2 and b"shape" in lib.hrn_last_error() and b"16..16384" in lib.hrn_last_error(), bad
        assert f(B=0) == -2 and f(V=0) == -2 and b"batch" in lib.hrn_last_error()
        for block in (0, 32, 96, 100, 4160, 8192, -64):
            assert f(block=block) == -2 and b"block" in lib.hrn_last_error() and b"multiple of 64" in lib.hrn_last_error(), block
        # B V tiles beyond 2^31 - 1: 65536 tiles a view; B V blocks beyond it where the tiles still fit needs B V itself beyond it
        assert f(B=1 << 15, V=1, H=16384, W=16384) == -2 and b"exceed one launch" in lib.hrn_last_error()
    assert search(P=2) == -2 and b"P=2" in lib.hrn_last_error()
    assert search(P=10) == -2 and b"P=10" in lib.hrn_last_error()
    assert search(ws=null) == -2 and b"null" in lib.hrn_last_error()
    assert search(field=null) == -2 and b"null" in lib.hrn_last_error()
    assert apply(out=null) == -2 and b"null" in lib.hrn_last_error()
    assert search(levels=0) == -2 and b"levels" in lib.hrn_last_error()
    assert search(levels=17) == -2
    assert search(radius=0.0) == -2 and b"radius" in lib.hrn_last_error()
    assert search(radius=4.5) == -2 and search(radius=float("nan")) == -2
    assert search(min_valid=-0.1) == -2 and b"min_valid" in lib.hrn_last_error()
    assert search(min_valid=1.5) == -2 and search(min_valid=float("nan")) == -2


def test_c_entry_point_refuses_a_workspace_one_byte_short(lib):
    _, _, _, search, _ = _calls(lib)
    for shape in (dict(), dict(H=16, W=16), dict(B=1, V=1, H=257, W=144, P=9, block=128), dict(block=4096)):
        assert search(short=1, **shape) == -3 and b"workspace" in lib.hrn_last_error(), shape


def test_workspace_size(lib):
    need = lib.hrn_mncc_local_workspace_bytes
    for bad in ((0, 1, 64, 64, 7, 64), (1, 0, 64, 64, 7, 64), (1, 1, 15, 64, 7, 64), (1, 1, 64, 16385, 7, 64), (1, 1, 64, 64, 2, 64),
                (1, 1, 64, 64, 10, 64), (1, 1, 64, 64, 7, 32), (1, 1, 64, 64, 7, 96), (1, 1, 64, 64, 7, 8192), (1 << 15, 1, 16384, 16384, 7, 64)):
        assert need(*bad) == 0, bad
    for B, V, H, W, P, block in ((1, 2, 16, 16, 7, 64), (1, 2, 130, 203, 7, 64), (1, 2, 257, 144, 9, 128), (2, 3, 200, 264, 3, 64),
                                 (2, 32, 512, 512, 7, 128), (1, 32, 8192, 6144, 9, 4096)):
        T, C = -(-H // 64) * -(-W // 64), min(64, -(-H * W // 16384))
        blocks = L.blocks(H, block) * L.blocks(W, block)
        assert need(B, V, H, W, P, block) == 16 * (B * V + B) * C + 48 * P * P * B * V * T + 8 * B * V * blocks, (B, V, H, W, P, block)
        # the scene search's workspace but for the centres: one pair per block instead of one per view
        assert need(B, V, H, W, P, block) - lib.hrn_mncc_scene_workspace_bytes(B, V, H, W, P) == 8 * B * V * (blocks - 1)


def test_fake_kernels_give_the_shapes():
    ops = torch.ops.hrnet_hip
    B, V, H, W = 2, 5, 200, 264
    views, masks = torch.empty(B, V, H, W, device="meta"), torch.empty(B, V, H, W, device="meta")
    ref, init = torch.empty(B, H, W, device="meta"), torch.empty(B, V, 2, device="meta")
    field, trace, ok = ops.mncc_search_local(ref, None, views, masks, init, 7, 4, 0.5, 64, 0.25)
    assert field.shape == (B, V, 3, 4, 2) and trace.shape == (B, V, 3, 4, 4, 3) and ok.shape == (B, V, 3, 4)
    assert field.dtype == trace.dtype == ok.dtype == torch.float32 and field.device.type == "meta"
    field, trace, ok = ops.mncc_search_local(ref, ref, views, None, None, 5, 2, 1.0, 4096, 0.0)
    assert field.shape == (B, V, 1, 1, 2) and trace.shape == (B, V, 1, 1, 2, 3) and ok.shape == (B, V, 1, 1)
    out, valid = ops.shift_field(views.double(), masks, torch.empty(B, V, 3, 4, 2, device="meta"), 64)
    assert out.shape == valid.shape == (B, V, H, W) and out.dtype == valid.dtype == torch.float32


def test_python_argument_errors():
    from hrnet_hip import registration as G
    a, m = torch.zeros(2, 3, 130, 203), torch.ones(2, 3, 130, 203)
    with pytest.raises(TypeError, match="torch.Tensor"):
        G.mncc_search_local(a.numpy())
    with pytest.raises(ValueError, match=r"\(B,V,H,W\).*\(2, 130, 203\)"):
        G.mncc_search_local(a[:, 0])
    with pytest.raises(ValueError, match=r"lr_masks.*\(2, 3, 130, 203\).*\(2, 3, 130, 16\)"):
        G.mncc_search_local(a, m[..., :16])
    with pytest.raises(ValueError, match=r"16\.\.16384.*\(8, 20\)"):
        G.mncc_search_local(torch.zeros(1, 2, 8, 20))
    with pytest.raises(ValueError, match=r"16\.\.16384.*\(16, 16385\)"):
        G.shift_field(torch.zeros(1, 1, 16, 16385), None, torch.zeros(1, 1, 1, 4, 2), 4096)
    with pytest.raises(ValueError, match=r"ref must be \(B,H,W\) = \(2, 130, 203\)"):
        G.mncc_search_local(a, ref=a[:, 0, :, :16])
    for bad, what in ((dict(points_per_dim=2), "points_per_dim"), (dict(points_per_dim=10), "points_per_dim"), (dict(levels=0), "levels"),
                      (dict(levels=17), "levels"), (dict(radius=0.0), "radius"), (dict(radius=4.1), "radius"), (dict(block=96), "block"),
                      (dict(block=32), "block"), (dict(block=8192), "block"), (dict(min_valid=-0.1), "min_valid"), (dict(min_valid=1.1), "min_valid")):
        with pytest.raises(ValueError, match=what):
            G.mncc_search_local(a, m, **bad)
    for bad, what in ((dict(local_levels=0), "levels"), (dict(local_radius=5.0), "radius"), (dict(block=100), "block"), (dict(min_valid=2.0), "min_valid"),
                      (dict(levels=17), "levels"), (dict(points_per_dim=2), "points_per_dim")):
        with pytest.raises(ValueError, match=what):
            G.register_scene_local(a, m, **bad)
    with pytest.raises(TypeError, match="init must be a torch.Tensor"):
        G.mncc_search_local(a, m, init=np.zeros((2, 3, 2)))
    with pytest.raises(ValueError, match=r"init.*\(2, 3, 2\).*\(2, 3\)"):
        G.mncc_search_local(a, m, init=torch.zeros(2, 3))
    with pytest.raises(TypeError, match="field must be a torch.Tensor"):
        G.shift_field(a, m, np.zeros((2, 3, 2, 3, 2)), 64)
    with pytest.raises(ValueError, match=r"field.*\(2, 3, 2, 3, 2\).*\(2, 3, 2\)"):
        G.shift_field(a, m, torch.zeros(2, 3, 2), 64)
    with pytest.raises(ValueError, match=r"field.*\(2, 3, 1, 2, 2\).*\(2, 3, 2, 3, 2\)"):
        G.shift_field(a, m, torch.zeros(2, 3, 2, 3, 2), 128)
    with pytest.raises(TypeError, match="trace"):
        G.register_scene_local(a, m, return_trace=True)
    for call in (lambda: G.mncc_search_local(a, m), lambda: G.mncc_search_local(a, m, init=torch.zeros(2, 3, 2)),
                 lambda: G.shift_field(a, m, torch.zeros(2, 3, 2, 3, 2), 64), lambda: G.register_scene_local(a)):
        with pytest.raises(TypeError, match="no CPU fallback"):
            call()


# ----------------------------------------------------------------------------- tools/registration_local_bench.py
def test_bench_tool_command_line():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import registration_local_bench as T
    assert "import _common" in open(T.__file__).read()
    assert vars(T.PARSER.parse_args([])) == dict(B=2, views=32, size=512, block=128, points=7, levels=6, local_levels=4, rounds=7, reps=5)
    got = vars(T.PARSER.parse_args("1 --views 4 --size 200 --block 64 --points 5 --levels 4 --local-levels 2 --rounds 3 --reps 2".split()))
    assert got == dict(B=1, views=4, size=200, block=64, points=5, levels=4, local_levels=2, rounds=3, reps=2)
    with pytest.raises(SystemExit) as e:
        T.PARSER.parse_args(["--bogus", "1"])
    assert e.value.code == 2
    with pytest.raises(SystemExit) as e:
        T.PARSER.parse_args(["--help"])
    assert e.value.code == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="there is a device: the tool would start measuring")
def test_bench_tool_refuses_to_run_without_a_device():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "registration_local_bench.py")], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 2 and "Traceback" not in r.stderr and r.stdout == ""
    assert r.stderr.strip().splitlines()[-1] == "registration_local_bench needs a ROCm device: a time cannot be measured without one"
