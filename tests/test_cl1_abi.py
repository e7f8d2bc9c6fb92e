"""CPU: the three C entry points of the shift-searched L1 / Charbonnier loss refuse bad arguments with a negative code before any launch
(no device is touched: the pointers below are never dereferenced), and the workspace query states the bytes."""
import ctypes
import os

import pytest


@pytest.fixture(scope="module")
def lib():
    from hrnet_hip import binding, build
    if not os.path.exists(binding.LIB_PATH):
        build.build_library(verbose=False)
    return binding.load_library()


B, H, W, BORDER = 2, 40, 56, 3
NULL = ctypes.c_void_p(0)


def _train(lib, p, **kw):
    a = dict(srs=p, hrs=p, maps=p, B=B, H=H, W=W, border=BORDER, clip=0, eps=0.0, out=p, stats=p, ws=p,
             ws_bytes=lib.hrn_cl1_loss_workspace_bytes(B, H, W, BORDER), stream=NULL)
    a.update(kw)
    return lib.hrn_cl1_loss_train(a["srs"], a["hrs"], a["maps"], a["B"], a["H"], a["W"], a["border"], a["clip"], a["eps"], a["out"], a["stats"],
                                  a["ws"], a["ws_bytes"], a["stream"])


def _backward(lib, p, **kw):
    a = dict(srs=p, hrs=p, maps=p, stats=p, d_out=p, B=B, H=H, W=W, border=BORDER, clip=0, eps=0.0, d_srs=p, stream=NULL)
    a.update(kw)
    return lib.hrn_cl1_loss_backward(a["srs"], a["hrs"], a["maps"], a["stats"], a["d_out"], a["B"], a["H"], a["W"], a["border"], a["clip"],
                                     a["eps"], a["d_srs"], a["stream"])


def test_workspace_bytes(lib):
    # 32 x 128 tiles of the (H - 2 border) x (W - 2 border) crop, two fp64 sums per tile and offset, and {n_k, b_k} per offset
    for (h, w, border), tiles in (((40, 56, 3), 2), ((20, 20, 0), 1), ((96, 96, 3), 3), ((40, 300, 8), 3), ((70, 139, 5), 4)):
        nk = (2 * border + 1) ** 2
        assert lib.hrn_cl1_loss_workspace_bytes(B, h, w, border) == B * (tiles + 1) * nk * 2 * 8
    for bad in ((0, H, W, 3), (B, H, W, -1), (B, H, W, 9), (B, 6, W, 3), (B, H, 6, 3), (70000, H, W, 3), (1, 65536, 32768, 0)):
        assert lib.hrn_cl1_loss_workspace_bytes(*bad) == 0


def test_bad_arguments_fail_before_any_launch(lib):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    for name in ("srs", "hrs", "maps", "out", "stats", "ws"):
        assert _train(lib, p, **{name: NULL}) == -2 and b"null" in lib.hrn_last_error()
    for name in ("srs", "hrs", "maps", "stats", "d_out", "d_srs"):
        assert _backward(lib, p, **{name: NULL}) == -2 and b"null" in lib.hrn_last_error()
    for call in (_train, _backward):
        assert call(lib, p, border=9) == -2 and b"border" in lib.hrn_last_error()
        assert call(lib, p, border=-1) == -2
        assert call(lib, p, H=2 * BORDER) == -2 and b"shape" in lib.hrn_last_error()
        assert call(lib, p, W=2 * BORDER) == -2
        assert call(lib, p, B=0) == -2
        assert call(lib, p, B=65536) == -2
        assert call(lib, p, H=65536, W=32768) == -2 and b"2^31" in lib.hrn_last_error()
        for eps in (-1e-3, float("nan"), float("inf")):
            assert call(lib, p, eps=eps) == -2 and b"eps" in lib.hrn_last_error()
    need = lib.hrn_cl1_loss_workspace_bytes(B, H, W, BORDER)
    assert need > 0 and _train(lib, p, ws_bytes=need - 1) == -3 and b"workspace" in lib.hrn_last_error()
    assert _train(lib, p, ws_bytes=0) == -3
