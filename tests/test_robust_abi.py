"""CPU: the C entry points of the robust data term and the bilateral-TV prior (csrc/robust_sr.hip) refuse bad arguments with -2 before
any launch (no device is touched: the pointers below are never dereferenced), and the workspace queries state the bytes."""
import ctypes
import os

import pytest


@pytest.fixture(scope="module")
def lib():
    from hrnet_hip import binding, build
    if not os.path.exists(binding.LIB_PATH):
        build.build_library(verbose=False)
    return binding.load_library()


NULL = ctypes.c_void_p(0)
P_ = [ctypes.c_void_p((k + 1) << 20) for k in range(8)]                   # eight buffers 1 MiB apart
B, V, H, W, SCALE = 1, 2, 4, 4, 3
BIG = 1 << 16


def _sums(lib, **kw):
    a = dict(residual=P_[0], masks=NULL, alphas=NULL, shifts=P_[1], beta_prev=P_[2], ws=P_[3], ws_bytes=BIG, B=B, V=V, H=H, W=W, scale=SCALE, delta=0.1)
    a.update(kw)
    return lib.hrn_robust_sums(a["residual"], a["masks"], a["alphas"], a["shifts"], a["beta_prev"], a["ws"], a["ws_bytes"], a["B"], a["V"], a["H"],
                               a["W"], a["scale"], a["delta"], NULL)


def _finish(lib, **kw):
    a = dict(ws=P_[3], ws_bytes=BIG, count=P_[0], beta=P_[1], inlier=P_[2], loss=P_[4], B=B, V=V, H=H, W=W)
    a.update(kw)
    return lib.hrn_robust_finish(a["ws"], a["ws_bytes"], a["count"], a["beta"], a["inlier"], a["loss"], a["B"], a["V"], a["H"], a["W"], 1, NULL)


def _apply(lib, **kw):
    a = dict(residual=P_[0], masks=NULL, alphas=NULL, shifts=P_[1], beta_prev=P_[2], beta=P_[3], weighted=P_[4], B=B, V=V, H=H, W=W, scale=SCALE,
             delta=0.1)
    a.update(kw)
    return lib.hrn_robust_apply(a["residual"], a["masks"], a["alphas"], a["shifts"], a["beta_prev"], a["beta"], a["weighted"], a["B"], a["V"],
                                a["H"], a["W"], a["scale"], a["delta"], NULL)


def _map(fn):
    def call(lib, **kw):
        a = dict(x=P_[0], c=P_[1], out=P_[2], planes=2, SH=20, SW=30, P=2, alpha=0.7, eps=0.02)
        a.update(kw)
        return getattr(lib, fn)(a["x"], a["c"], a["out"], a["planes"], a["SH"], a["SW"], a["P"], a["alpha"], a["eps"], NULL)
    return call


def _value(lib, **kw):
    a = dict(x=P_[0], value=P_[1], ws=P_[2], ws_bytes=BIG, planes=2, SH=20, SW=30, P=2, alpha=0.7, eps=0.02, gain=1.0)
    a.update(kw)
    return lib.hrn_btv_value(a["x"], a["value"], a["ws"], a["ws_bytes"], a["planes"], a["SH"], a["SW"], a["P"], a["alpha"], a["eps"], a["gain"], NULL)


def test_constants_and_workspace_bytes(lib):
    from hrnet_hip import binding
    assert binding.BTV_TILE == (16, 64) and binding.BTV_MAX_P == 3 and binding.BTV_MAX_SIDE == 49152 == 3 * binding.OBSERVE_MAX_SIDE
    for shape in [(1, 1, 1, 1), (2, 5, 17, 63), (32, 32, 128, 128), (1, 1, 16384, 16384)]:
        assert lib.hrn_robust_workspace_bytes(*shape) == lib.hrn_observe_workspace_bytes(*shape) > 0      # three fp64 sums per LR tile
    for shape in [(0, 1, 8, 8), (1, 0, 8, 8), (1, 1, 0, 8), (1, 1, 8, 16385), (-1, 1, 8, 8)]:
        assert lib.hrn_robust_workspace_bytes(*shape) == 0
    for (n, sh, sw), tiles in (((1, 1, 1), 1), ((3, 16, 64), 1), ((3, 17, 64), 2), ((3, 16, 65), 2), ((2, 33, 129), 9), ((1, 49152, 49152), 3072 * 768)):
        assert lib.hrn_btv_workspace_bytes(n, sh, sw) == 8 * n * tiles                                   # one fp64 sum per 16 x 64 tile
    for bad in [(0, 8, 8), (1, 0, 8), (1, 8, 0), (1, 49153, 8), (1, 8, 49153), (-1, 8, 8)]:
        assert lib.hrn_btv_workspace_bytes(*bad) == 0


def test_robust_entry_points_refuse_bad_arguments(lib):
    required = ((_sums, ("residual", "shifts", "beta_prev", "ws")), (_finish, ("ws", "count", "beta", "inlier", "loss")),
                (_apply, ("residual", "shifts", "beta_prev", "beta", "weighted")))
    for fn, ptrs in required:
        for name in ptrs:
            assert fn(lib, **{name: NULL}) == -2 and b"null" in lib.hrn_last_error(), name
        for name in ("B", "V", "H", "W"):
            assert fn(lib, **{name: 0}) == -2 and b"empty" in lib.hrn_last_error(), name
            assert fn(lib, **{name: -3}) == -2, name
        assert fn(lib, H=16385) == -2 and b"16384" in lib.hrn_last_error()
        assert fn(lib, W=16385) == -2
    for fn in (_sums, _apply):
        for scale in (1, 5, 0):
            assert fn(lib, scale=scale) == -2 and b"scale" in lib.hrn_last_error()
        for delta in (0.0, -0.1, float("nan"), float("inf")):
            assert fn(lib, delta=delta) == -2 and b"delta" in lib.hrn_last_error(), delta
    need = lib.hrn_robust_workspace_bytes(B, V, H, W)
    for fn in (_sums, _finish):
        assert fn(lib, ws_bytes=need - 1) == -2 and b"workspace" in lib.hrn_last_error()
        assert fn(lib, ws=ctypes.c_void_p((4 << 20) + 4)) == -2 and b"aligned" in lib.hrn_last_error()
    assert _sums(lib, ws=P_[0]) == -2 and b"alias" in lib.hrn_last_error()
    assert _sums(lib, ws=P_[2]) == -2 and b"alias" in lib.hrn_last_error()
    assert _finish(lib, beta=P_[3]) == -2 and b"alias" in lib.hrn_last_error()
    assert _finish(lib, inlier=P_[1]) == -2 and b"alias" in lib.hrn_last_error()
    assert _finish(lib, loss=P_[0]) == -2 and b"alias" in lib.hrn_last_error()
    assert _apply(lib, weighted=P_[0]) == -2 and b"alias" in lib.hrn_last_error()
    assert _apply(lib, weighted=P_[3]) == -2 and b"alias" in lib.hrn_last_error()


def test_btv_entry_points_refuse_bad_arguments(lib):
    step, backward = _map("hrn_btv_step"), _map("hrn_btv_backward")
    for fn, ptrs in ((step, ("x", "c", "out")), (backward, ("x", "c", "out")), (_value, ("x", "value", "ws"))):
        for name in ptrs:
            assert fn(lib, **{name: NULL}) == -2 and b"null" in lib.hrn_last_error(), name
        for name in ("planes", "SH", "SW"):
            assert fn(lib, **{name: 0}) == -2 and b"empty" in lib.hrn_last_error(), name
            assert fn(lib, **{name: -1}) == -2, name
        assert fn(lib, SH=49153) == -2 and b"49152" in lib.hrn_last_error()
        assert fn(lib, SW=49153) == -2
        for P in (0, 4, -1):
            assert fn(lib, P=P) == -2 and b"P must" in lib.hrn_last_error(), P
        for alpha in (0.0, -0.5, 1.5, float("nan"), float("inf")):
            assert fn(lib, alpha=alpha) == -2 and b"alpha" in lib.hrn_last_error(), alpha
        for eps in (0.0, -0.02, float("nan"), float("inf")):
            assert fn(lib, eps=eps) == -2 and b"eps" in lib.hrn_last_error(), eps
    # a stencil: out may not be x, nor overlap it
    for fn in (step, backward):
        assert fn(lib, out=P_[0]) == -2 and b"alias" in lib.hrn_last_error()
        assert fn(lib, out=ctypes.c_void_p((1 << 20) + 16)) == -2 and b"alias" in lib.hrn_last_error()
        assert fn(lib, out=P_[1]) == -2 and b"alias" in lib.hrn_last_error()
    need = lib.hrn_btv_workspace_bytes(2, 20, 30)
    assert need == 8 * 2 * 2
    assert _value(lib, ws_bytes=need - 1) == -2 and b"workspace" in lib.hrn_last_error()
    assert _value(lib, ws=ctypes.c_void_p((3 << 20) + 4)) == -2 and b"aligned" in lib.hrn_last_error()
    assert _value(lib, ws=P_[0]) == -2 and b"alias" in lib.hrn_last_error()
    assert _value(lib, value=P_[0]) == -2 and b"alias" in lib.hrn_last_error()
    for gain in (float("nan"), float("inf")):
        assert _value(lib, gain=gain) == -2 and b"gain" in lib.hrn_last_error()
