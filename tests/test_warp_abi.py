"""CPU: the two C entry points of the sampler's backward are declared, exported and bound with the declared types, refuse bad arguments
with a negative code before any launch (no device is touched: the pointers below are never dereferenced), and the workspace query
states the bytes."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, V, H, W = 2, 3, 130, 203
NULL = ctypes.c_void_p(0)


@pytest.fixture(scope="module")
def lib():
    from hrnet_hip import binding, build
    if not os.path.exists(binding.LIB_PATH):
        build.build_library(verbose=False)
    return binding.load_library()


def _tiles(h, w):
    return ((h + 63) // 64) * ((w + 63) // 64)


def _call(lib, p, **kw):
    a = dict(views=p, shifts=p, valid=p, d_out=p, B=B, V=V, H=H, W=W, d_views=p, d_shifts=p, ws=p,
             ws_bytes=lib.hrn_mncc_apply_backward_workspace_bytes(B, V, H, W), stream=NULL)
    a.update(kw)
    return lib.hrn_mncc_apply_backward(a["views"], a["shifts"], a["valid"], a["d_out"], a["B"], a["V"], a["H"], a["W"], a["d_views"],
                                       a["d_shifts"], a["ws"], a["ws_bytes"], a["stream"])


def test_declared_exported_and_bound_with_the_declared_types(lib):
    from hrnet_hip import binding
    c = ctypes
    header = open(os.path.join(ROOT, "include", "hrnet_hip.h")).read()
    assert re.search(r"^size_t hrn_mncc_apply_backward_workspace_bytes\(int B, int V, int H, int W\);", header, re.M)
    assert re.search(r"^int hrn_mncc_apply_backward\(const float\* views, const float\* shifts, const float\* valid, const float\* d_out,\s+"
                     r"int B, int V, int H, int W,\s+float\* d_views, float\* d_shifts,\s+void\* workspace, size_t workspace_bytes, "
                     r"void\* stream\);", header, re.M)
    assert binding.SIGNATURES["hrn_mncc_apply_backward_workspace_bytes"] == (c.c_size_t, [c.c_int] * 4)
    assert binding.SIGNATURES["hrn_mncc_apply_backward"] == (c.c_int, [c.c_void_p] * 4 + [c.c_int] * 4 + [c.c_void_p] * 3
                                                             + [c.c_size_t, c.c_void_p])
    for name in ("hrn_mncc_apply_backward_workspace_bytes", "hrn_mncc_apply_backward"):
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == binding.SIGNATURES[name]
    assert "resample_bwd.hip" in __import__("hrnet_hip.build", fromlist=["SOURCES"]).SOURCES


def test_workspace_bytes(lib):
    for b, v, h, w in ((1, 2, 24, 40), (1, 3, 33, 47), (2, 2, 130, 203), (2, 32, 512, 512), (1, 1, 16, 16), (1, 1, 16384, 16384), (3, 5, 64, 65)):
        assert lib.hrn_mncc_apply_backward_workspace_bytes(b, v, h, w) == 16 * b * v * _tiles(h, w)
    for bad in ((0, V, H, W), (B, 0, H, W), (-1, V, H, W), (B, -2, H, W), (B, V, 15, W), (B, V, H, 15), (B, V, 16385, W), (B, V, H, 16385),
                (65536, 65536, H, W), (4096, 4096, 16384, 16384)):
        assert lib.hrn_mncc_apply_backward_workspace_bytes(*bad) == 0


def test_bad_arguments_fail_before_any_launch(lib):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    for name in ("views", "shifts", "valid", "d_out", "ws"):
        assert _call(lib, p, **{name: NULL}) == -2 and b"null" in lib.hrn_last_error()
    assert _call(lib, p, d_views=NULL, d_shifts=NULL) == -2 and b"both null" in lib.hrn_last_error()
    # without d_shifts neither the views nor the workspace is required, but the rest is
    for name in ("shifts", "valid", "d_out"):
        assert _call(lib, p, d_shifts=NULL, views=NULL, ws=NULL, ws_bytes=0, **{name: NULL}) == -2 and b"null" in lib.hrn_last_error()
    for side in (15, 16385):
        assert _call(lib, p, H=side) == -2 and b"shape" in lib.hrn_last_error()
        assert _call(lib, p, W=side) == -2 and b"shape" in lib.hrn_last_error()
    for n in (0, -1):
        assert _call(lib, p, B=n) == -2 and b"batch" in lib.hrn_last_error()
        assert _call(lib, p, V=n) == -2 and b"batch" in lib.hrn_last_error()
    assert _call(lib, p, B=4096, V=4096, H=16384, W=16384) == -2 and b"exceed one launch" in lib.hrn_last_error()
    need = lib.hrn_mncc_apply_backward_workspace_bytes(B, V, H, W)
    assert need == 16 * B * V * 12
    assert _call(lib, p, ws_bytes=need - 1) == -3 and b"workspace" in lib.hrn_last_error()
    assert _call(lib, p, ws_bytes=0) == -3
    # the shape is judged before the pointers
    assert _call(lib, p, H=15, views=NULL) == -2 and b"shape" in lib.hrn_last_error()
