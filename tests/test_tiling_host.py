"""CPU: tiled inference as far as it lives on the host - the window rule of hrnet_hip/tiling.py (halo, axis_plan, plan, gather,
scatter), its exactness end to end on the CPU port of the network (tiled == whole frame with the halo at R, and visibly not with
R - 1: the formula is sufficient and not padded), the refusals of hrn_tile_gather / hrn_tile_scatter / hrn_tile_count /
hrn_hrnet_halo (nothing is launched), the fake kernels of the two dispatcher ops and the `tile` attribute."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from hrnet_hip import tiling
from oracle import synth, torch_port, weights
import util

FP32_GUARD = 2e-5            # the project's fp32 regression bound (tests/test_gpu_parity.py), max-rel


# --------------------------------------------------------------------------- the rule
def test_halo():
    assert tiling.halo(2, 32) == 21 and tiling.halo(2, 4) == 12 and tiling.halo(2, 5) == 12 and tiling.halo(2, 2) == 9
    assert tiling.halo(2, 9) == 15 and tiling.halo(2, 1) == 6 and tiling.halo(0, 1) == 2 and tiling.halo(8, 3) == 21
    for v in range(1, 70):
        assert tiling.halo(2, v) == 6 + 3 * int(math.floor(math.log2(v)))
    for bad in ((-1, 4), (2, 0)):
        with pytest.raises(ValueError):
            tiling.halo(*bad)


def _sweep():
    """(L, t, R): L == t, L == t + 1, k == 1 (t == 2R + 1), last windows clamped at the far border, exact fits, R == 0."""
    cases = []
    for R in (0, 1, 2, 5, 12, 21):
        for t in sorted({2 * R + 1, 2 * R + 2, 2 * R + 3, 2 * R + 8, 3 * R + 5, 48}):
            if t < 2 * R + 1:
                continue
            k = t - 2 * R
            for L in sorted({t, t + 1, t + 2, t + k - 1, t + k, t + k + 1, t + 3 * k, t + 3 * k + 1, 2 * t, 2 * t + 1, 5 * t - 3, 131}):
                if L >= t:
                    cases.append((L, t, R))
    return cases


def test_axis_plan_properties():
    cases = _sweep()
    assert len(cases) > 300
    clamped = 0
    for L, t, R in cases:
        ws = tiling.axis_plan(L, t, R)
        k = t - 2 * R
        assert len(ws) == tiling.axis_count(L, t, R) == (1 if L == t else math.ceil((L - 2 * R) / k)), (L, t, R)
        assert ws[0][1] == 0 and ws[-1][2] == L
        for i, (start, lo, hi) in enumerate(ws):
            assert 0 <= start and start + t <= L, (L, t, R, i)                                 # inside the scene
            assert start <= lo < hi <= start + t                                                # a non-empty core inside its window
            assert lo == 0 if i == 0 else lo == ws[i - 1][2]                                    # the cores partition [0, L)
            assert lo == 0 or lo - start >= R, (L, t, R, i)                                     # on the border, or R inside the window
            assert hi == L or start + t - hi >= R, (L, t, R, i)
            if i >= 1:
                assert lo == (t - R) + (i - 1) * k
            clamped += i >= 1 and start != lo - R
        if L == t + 1:
            assert ws == [(0, 0, t - R), (1, t - R, L)]
    assert clamped > 50                                                                         # the far-border clamp was exercised
    assert tiling.axis_plan(7, 7, 30) == [(0, 0, 7)]                                            # one window: any halo
    for bad in ((10, 11, 1), (10, 4, 2), (10, 0, 0), (10, 5, -1), (10.0, 5, 1)):
        with pytest.raises(ValueError):
            tiling.axis_plan(*bad)


def test_plan_properties_and_refusals():
    for H, W, tile, R in ((40, 56, 32, 12), (44, 44, 36, 12), (24, 37, 20, 9), (48, 33, 33, 15), (33, 48, 64, 15), (512, 512, 128, 21),
                          (512, 512, 256, 21), (2048, 1536, 128, 21), (5, 5, 128, 21), (1, 9, 4, 0)):
        p = tiling.plan(H, W, tile, R)
        t = min(tile, H, W)
        assert (p.H, p.W, p.t, p.R) == (H, W, t, R) and len(p.windows) == p.ny * p.nx
        assert p.ny == tiling.axis_count(H, t, R) and p.nx == tiling.axis_count(W, t, R)
        assert p.overhead == len(p.windows) * t * t / (H * W)
        cover = np.zeros((H, W), np.int32)
        for i, w in enumerate(p.windows):
            assert 0 <= w.y0 and w.y0 + t <= H and 0 <= w.x0 and w.x0 + t <= W
            cover[w.cy0:w.cy1, w.cx0:w.cx1] += 1
            assert (w.y0, w.cy0, w.cy1) == tiling.axis_plan(H, t, R)[i // p.nx] and (w.x0, w.cx0, w.cx1) == tiling.axis_plan(W, t, R)[i % p.nx]
        assert (cover == 1).all()                                                               # every pixel in exactly one core
    assert [len(tiling.plan(*a).windows) for a in ((40, 56, 32, 12), (44, 44, 36, 12), (24, 37, 20, 9), (48, 33, 33, 15))] == [8, 4, 30, 6]
    assert tiling.plan(512, 512, 128, 21).overhead == 2.25 and tiling.plan(512, 512, 256, 21).overhead == 2.25
    assert len(tiling.plan(512, 512, 256, 21).windows) == 9 and len(tiling.plan(512, 512, 128, 21).windows) == 36
    assert len(tiling.plan(30, 30, 64, 21).windows) == 1                                        # a single window: always allowed
    for H, W, tile, R in ((40, 56, 24, 12), (64, 64, 42, 21), (30, 31, 64, 21)):
        with pytest.raises(ValueError) as e:
            tiling.plan(H, W, tile, R)
        for word in (f"H={H}", f"W={W}", f"tile={tile}", f"R={R}"):
            assert word in str(e.value), str(e.value)
    for bad in ((0, 8, 4, 1), (8, 8, 0, 1), (8, 8, 4, -1), (8, 8, 4.0, 1)):
        with pytest.raises(ValueError):
            tiling.plan(*bad)


def test_gather_and_scatter_are_plain_indexing():
    g = np.random.Generator(np.random.PCG64(3))
    p = tiling.plan(24, 37, 20, 9)
    x = torch.from_numpy(g.standard_normal((2, 3, 24, 37)).astype(np.float32))
    wins = tiling.gather(x, p.windows, p.t)
    assert tuple(wins.shape) == (30, 2, 3, 20, 20)
    for i, w in enumerate(p.windows):
        assert torch.equal(wins[i], x[:, :, w.y0:w.y0 + 20, w.x0:w.x0 + 20])
    # scattering windows cut from one SR plane gives that plane back; a sub-range touches its cores only
    for S in (2, 3, 4):
        big = torch.from_numpy(g.standard_normal((2, 1, S * 24, S * 37)).astype(np.float32))
        srs = torch.stack([big[:, :, S * w.y0:S * (w.y0 + 20), S * w.x0:S * (w.x0 + 20)] for w in p.windows])
        out = torch.full_like(big, float("nan"))
        assert tiling.scatter(out, srs, p.windows, 20, S) is out and torch.equal(out, big)
        part = torch.full_like(big, float("nan"))
        tiling.scatter(part, srs[7:19], p.windows[7:19], 20, S)
        mask = torch.zeros((S * 24, S * 37), dtype=torch.bool)
        for w in p.windows[7:19]:
            mask[S * w.cy0:S * w.cy1, S * w.cx0:S * w.cx1] = True
        assert torch.equal(torch.isfinite(part), mask.expand_as(part)) and torch.equal(part[:, :, mask], big[:, :, mask])
    with pytest.raises(ValueError):
        tiling.scatter(out, srs[:3], p.windows, 20, 4)


# --------------------------------------------------------------------------- exactness on the CPU port of the network
ROWS = [(4, 40, 56, 32, 12, 8), (5, 44, 44, 36, 12, 4), (2, 24, 37, 20, 9, 30), (9, 48, 33, 33, 15, 6)]      # V, H, W, tile, R, windows
_cache = {}


def _scene(V, H, W):
    """(lrs (1,V,H,W), alphas, state dict, the whole-frame prediction): computed once per row, shared, never modified."""
    key = (V, H, W)
    if key not in _cache:
        lrs, alphas, _ = synth.make_batch(100 + V, 1, V, max(H, W), V)
        x, a = torch.from_numpy(np.ascontiguousarray(lrs[:, :, :H, :W])), torch.from_numpy(alphas)
        st = weights.to_torch_state(weights.hrnet_state(1234))
        _cache[key] = (x, a, st, torch_port.hrnet_forward(x, a, st))
    return _cache[key]


def _tiled(x, a, st, tile, R):
    p = tiling.plan(x.shape[2], x.shape[3], tile, R)
    wins = tiling.gather(x, p.windows, p.t)
    srs = torch.stack([torch_port.hrnet_forward(w.contiguous(), a, st) for w in wins])
    return tiling.scatter(torch.full((1, 1, 3 * x.shape[2], 3 * x.shape[3]), float("nan")), srs, p.windows, p.t, 3), p


@pytest.mark.parametrize("V,H,W,tile,R,n", ROWS, ids=lambda v: str(v))
def test_tiled_equals_whole_frame_on_the_cpu_port(V, H, W, tile, R, n):
    """gather -> the port's forward per window -> scatter against the port's forward of the whole (rectangular) frame, held to the
    fp32 guard (oneDNN may pick kernels by shape, so no bit equality is demanded on a CPU)."""
    x, a, st, whole = _scene(V, H, W)
    assert tiling.halo(weights.HRNET_CONFIG["encoder"]["num_layers"], V) == R
    got, p = _tiled(x, a, st, tile, R)
    assert len(p.windows) == n and tuple(got.shape) == tuple(whole.shape) == (1, 1, 3 * H, 3 * W)
    e = util.rel_err(got.numpy(), whole.numpy())
    print(f"V={V} {H}x{W} tile {tile} R={R}: {n} windows, overhead {p.overhead:.2f}, tiled vs whole max-rel {e:.2e}")
    assert torch.isfinite(got).all() and e <= FP32_GUARD, e


@pytest.mark.parametrize("V,H,W,tile,R,n", [ROWS[0], ROWS[2]], ids=lambda v: str(v))
def test_a_halo_one_pixel_short_is_visible(V, H, W, tile, R, n):
    """The formula is not padded: with R - 1 the seams show, by more than 10x the bound the exact halo is held to."""
    x, a, st, whole = _scene(V, H, W)
    got, _ = _tiled(x, a, st, tile, R - 1)
    e = util.rel_err(got.numpy(), whole.numpy())
    print(f"V={V} {H}x{W} tile {tile} halo R-1={R - 1}: tiled vs whole max-rel {e:.2e}")
    assert e > FP32_GUARD, e


# --------------------------------------------------------------------------- the C ABI's refusals
@pytest.fixture(scope="module")
def lib():
    from hrnet_hip import binding, build
    if not os.path.exists(binding.LIB_PATH):
        build.build_library(verbose=False)
    return binding.load_library()


def test_halo_and_count_match_the_rule(lib):
    for nl in range(0, 9):
        for v in (1, 2, 3, 4, 5, 9, 31, 32, 33, 64):
            assert lib.hrn_hrnet_halo(nl, v) == tiling.halo(nl, v)
    assert lib.hrn_hrnet_halo(9, 4) == -2 and lib.hrn_hrnet_halo(-1, 4) == -2
    assert lib.hrn_hrnet_halo(2, 0) == -2 and b"hrn_hrnet_halo" in lib.hrn_last_error()
    for L, t, R in _sweep():
        assert lib.hrn_tile_count(L, t, t, R) == tiling.axis_count(L, t, R), (L, t, R)
        assert lib.hrn_tile_count(t, L, t, R) == tiling.axis_count(L, t, R), (L, t, R)
    for H, W, tile, R in ((40, 56, 32, 12), (24, 37, 20, 9), (48, 33, 33, 15), (2048, 1536, 128, 21), (30, 30, 30, 21)):
        assert lib.hrn_tile_count(H, W, tile, R) == len(tiling.plan(H, W, tile, R).windows)


def test_refusals_before_any_launch(lib):
    """Every refusal returns -2 with a message that names the fault.  Nothing is launched: the pointers below are host memory."""
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def gather(x=p, out=p, B=1, V=2, H=40, W=56, t=32, R=12, w0=0, w1=8):
        return lib.hrn_tile_gather(x, B, V, H, W, t, R, w0, w1, out, None), lib.hrn_last_error()

    def scatter(x=p, out=p, B=1, H=40, W=56, t=32, R=12, scale=3, w0=0, w1=8):
        return lib.hrn_tile_scatter(x, B, H, W, t, R, scale, w0, w1, out, None), lib.hrn_last_error()

    for fn, call in ((b"hrn_tile_gather", gather), (b"hrn_tile_scatter", scatter)):
        for kw, word in (({"x": None}, b"null"), ({"out": None}, b"null"),
                         ({"t": 41}, b"exceeds the scene"), ({"t": 57}, b"exceeds the scene"),
                         ({"t": 24}, b"at least 2R+1 = 25"), ({"R": 16}, b"at least 2R+1 = 33"),
                         ({"w1": 9}, b"outside the plan's [0, 8)"), ({"w0": -1}, b"outside the plan"), ({"w0": 3, "w1": 3}, b"outside the plan"),
                         ({"w0": 8, "w1": 9}, b"outside the plan"),
                         ({"H": 0}, b"bad geometry"), ({"t": 0}, b"bad geometry"), ({"R": -1}, b"bad geometry"), ({"B": 0}, b"bad shape"),
                         ({"H": 60000, "W": 60000}, b"32-bit in-plane offsets")):
            rc, msg = call(**kw)
            assert rc == -2 and fn in msg and word in msg, (fn, kw, rc, msg)
    rc, msg = gather(V=0)
    assert rc == -2 and b"bad shape" in msg
    for s in (1, 5):
        rc, msg = scatter(scale=s)
        assert rc == -2 and b"scale must be 2, 3 or 4" in msg
    rc, msg = scatter(H=20000, W=20000, t=128, R=21, scale=4, w1=1)           # fits at x1, not at x4
    assert rc == -2 and b"32-bit in-plane offsets" in msg
    for args, word in (((40, 56, 41, 12), b"exceeds the scene"), ((40, 56, 24, 12), b"at least 2R+1"), ((0, 56, 24, 12), b"bad geometry")):
        assert lib.hrn_tile_count(*args) == -2 and b"hrn_tile_count" in lib.hrn_last_error() and word in lib.hrn_last_error()


def test_python_binding_refuses():
    from hrnet_hip import binding
    x = torch.zeros(1, 2, 40, 56)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        binding.tile_gather(x, 32, 12, 0, 8)                                   # a host tensor: no quiet fall-back
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        binding.tile_scatter(torch.zeros(1, 1, 120, 168), torch.zeros(8, 1, 1, 96, 96), 32, 12, 3, 0, 8)
    with pytest.raises(binding.HrnetHipError, match="at least 2R"):
        binding.tile_count(40, 56, 24, 12)
    assert binding.tile_count(40, 56, 32, 12) == 8 and binding.hrnet_halo(2, 32) == 21
    with pytest.raises(binding.HrnetHipError):
        binding.hrnet_halo(2, 0)


def test_fake_kernels_infer_shapes():
    from hrnet_hip import binding  # noqa: F401  (registers the ops)
    ops = torch.ops.hrnet_hip
    lrs = torch.empty((2, 4, 40, 56), device="meta")
    w = ops.tile_gather(lrs, 32, 12, 2, 7)
    assert tuple(w.shape) == (5, 2, 4, 32, 32) and w.dtype == torch.float32 and w.device.type == "meta"
    out = torch.empty((2, 1, 120, 168), device="meta")
    assert ops.tile_scatter(out, torch.empty((5, 2, 1, 96, 96), device="meta"), 32, 12, 3, 2, 7) is None
    assert "Tensor(a0!) out" in str(ops.tile_scatter.default._schema)           # the mutated argument is declared


def test_hrnet_tile_attribute_and_arguments():
    from DeepNetworks.HRNet import HRNet
    m = HRNet(weights.HRNET_CONFIG)
    assert m.tile is None and HRNet(dict(weights.HRNET_CONFIG, tile=96)).tile == 96
    x, a = torch.zeros(1, 4, 40, 56), torch.ones(1, 4)
    for bad in (0, -3, 2.0, True, "128"):
        with pytest.raises(ValueError, match="tile"):
            m.forward_tiled(x, a, tile=bad)
    for bad in (0, 1.5, True):
        with pytest.raises(ValueError, match="windows_per_pass"):
            m.forward_tiled(x, a, tile=32, windows_per_pass=bad)
    with pytest.raises(ValueError, match="members_per_pass"):
        m.forward_tiled(x, a, tile=32, ensemble="flip", members_per_pass=5)
    with pytest.raises(ValueError):
        m.forward_tiled(x, a, tile=32, ensemble="rot90")
    with pytest.raises(ValueError, match="alphas"):
        m.forward_tiled(x, torch.ones(1, 3), tile=32)
    with pytest.raises(ValueError) as e:                                        # R = 12 for 4 views: 24 < 25
        m.forward_tiled(x, a, tile=24)
    assert all(word in str(e.value) for word in ("H=40", "W=56", "tile=24", "R=12"))
    m.tile = 0
    with pytest.raises(ValueError, match="tile"):
        m.eval()(x, a)
