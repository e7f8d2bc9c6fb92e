"""CPU: the in-image limits tests/test_gpu_large_offsets.py exercises on the GPU, where they can be seen without a launch - a refused
value returns -2 with its message before anything is launched (the pointers below are host memory) -, and the helper that picks which
images of a multi-GiB tensor are checked, and the strip reference of the big-frame cases against the whole-image reference."""
import ctypes
import os

import pytest
import torch

import kernel_refs as K
import kt
from kernel_bounds import boundary_images, crossed, crossings
from kt import BF16, BF16X3


@pytest.fixture(scope="module")
def lib():
    """the library, built first where it is missing (as tests/test_tiling_host.py does); one that exists and does not load is a failure"""
    from hrnet_hip import binding, build
    if not os.path.exists(binding.LIB_PATH):
        build.build_library(verbose=False)
    return kt.lib()


def _conv_x3(lib, cin, cout, H, W):
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    rc = lib.hrn_kt_conv3x3_epi(BF16X3, 0, cin, cout, p, None, 0, 0, 0, p, p, None, None, 0, 0, None, 0, p, 0, 0, 64, 0, 64, 0, 1, H, W, None)
    return rc, lib.hrn_last_error()


def test_v6x3_limit_counts_the_wider_of_input_and_output(lib):
    """conv3x3_v6's 32-bit in-image offsets cover the OUTPUT image too: 64 -> 128 (the data gradient of a 128 -> 64 layer) writes 256 bytes
    per pixel, so H W 256 >= 2^31 is refused although its input image is half that.  (The guard counted 2 cin bytes per pixel only; such an
    image was accepted, and past 2^31 output bytes the out-of-image lanes of a ragged tile, marked by bit 31 of their offset, stored into
    the image.)"""
    for cin, cout, H, W in ((64, 128, 2048, 4096), (64, 128, 2049, 4095), (64, 128, 4095, 4096), (128, 64, 2048, 4096), (128, 128, 2048, 4096),
                            (64, 64, 4096, 4096)):
        rc, msg = _conv_x3(lib, cin, cout, H, W)
        assert rc == -2 and b"conv3x3 bf16x3: image too large for 32-bit in-image offsets" in msg and f"H={H} W={W}".encode() in msg, (cin, cout, H, W, rc, msg)


def test_wgrad_x3_and_stem_limits(lib):
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    lib.hrn_kt_launch_count_reset()
    for dt in (BF16, BF16X3):
        rc = lib.hrn_kt_conv_wgrad(dt, p, None, 0, 0, 0, p, 1, 2048, 4096, 64, 64, p, p, None)
        assert rc == -2 and b"conv_wgrad_x3: image too large for 32-bit in-image offsets (H=2048 W=4096)" in lib.hrn_last_error()
        rc = lib.hrn_kt_stem(dt, p, 1, p, 1, 1, None, p, p, None, p, 64, 1 << 16, 1 << 15, 1, None)
        assert rc == -2 and b"exceed the 32-bit segment count" in lib.hrn_last_error()
    rc = lib.hrn_kt_stem_dgrad_route(BF16, p, p, p, p, p, p, 1 << 30, 1, 9, 1, None)
    assert rc == -2 and b"exceed the grid" in lib.hrn_last_error()
    # the frame given from outside: the same grid, the same limit, whichever outputs are wanted; and no output wanted at all
    for d_lrs, d_ref in ((p, p), (p, None), (None, p)):
        rc = lib.hrn_kt_stem_dgrad_ref(BF16, p, p, p, d_lrs, d_ref, 1 << 30, 1, 9, 1, None)
        assert rc == -2 and b"stem dgrad: 1073741824 samples of 9 x 1 exceed the grid" in lib.hrn_last_error()
    rc = lib.hrn_kt_stem_dgrad_ref(BF16, p, p, p, None, None, 1, 1, 9, 1, None)
    assert rc == -2 and b"neither d_lrs nor d_ref is wanted" in lib.hrn_last_error()
    assert lib.hrn_kt_launch_count(b"conv_general") == 0 and lib.hrn_kt_launch_count(b"stem_wgrad") == 0


def test_boundary_images():
    per = 64 * 64 * 64
    assert crossings(8194 * per, 2) == [1 << 30, 1 << 31] and crossed(8194 * per, 2) == ["2^31B", "2^32B", "2^31el"]
    # 2-byte storage, power-of-two images: every crossing falls between two images, and both are checked
    assert boundary_images(8194, per, 2) == [0, 4095, 4096, 8191, 8192, 8193]
    # f32: byte 2^31, byte 2^32 and element 2^31 are three places
    assert boundary_images(8194, per, 4) == [0, 2047, 2048, 4095, 4096, 8191, 8192, 8193]
    assert crossed(4098 * per, 4) == ["2^31B", "2^32B"]
    # ragged images straddle their crossings
    per = 33 * 50 * 64
    got = boundary_images(20338, per, 2)
    assert got == [0, 10168, 20336, 20337]
    for e, m in ((1 << 30, 10168), (1 << 31, 20336)):
        assert m * per < e < (m + 1) * per
    assert boundary_images(3, per, 2) == [0, 2] and crossed(3 * per, 2) == []


@pytest.mark.parametrize("res_mode", [0, 1, 2, 3])
def test_ref_conv_rows_is_ref_conv_epi(res_mode):
    """kernel_refs.ref_conv_rows, the strip reference of regime B, against ref_conv_epi, the reference of every small-shape test: the whole
    image (y0 = 0, y1 = H: zero rows as halo) and interior / border strips with their real neighbour rows, for every residual mode"""
    g = torch.Generator().manual_seed(7 + res_mode)
    H, W, cin, cout = 13, 37, 128, (64 if res_mode == 3 else 128)
    geo = dict(n=2, half=1, pair_last=1)
    x = torch.randn((1, H, W, cin), generator=g, dtype=torch.float64)
    w = torch.randn((cout, cin, 3, 3), generator=g, dtype=torch.float64) * 0.05
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    stack = torch.randn((1, 2, H, W, 64), generator=g, dtype=torch.float64)
    res = torch.randn((1, H, W, cout), generator=g, dtype=torch.float64)
    alph = torch.tensor([[0.25, 0.75]])
    want, T = K.ref_conv_epi(x=x, w=w, b=b, slope=-0.3, res_mode=res_mode, res=res, stack=stack, geo=geo, alph=alph)
    rows = {0: None, 1: res[0], 2: torch.cat([stack[0, 0], stack[0, 1]], -1), 3: stack[0, 0]}[res_mode]
    for y0, y1 in ((0, H), (0, 5), (4, 9), (8, H)):
        xpad = torch.zeros((y1 - y0 + 2, W, cin), dtype=torch.float64)
        a, c = max(0, y0 - 1), min(H, y1 + 1)
        xpad[a - (y0 - 1):a - (y0 - 1) + c - a] = x[0, a:c]
        got, Tg = K.ref_conv_rows(xpad, w, b, -0.3, res_mode, None if rows is None else rows[y0:y1], 0.75)
        assert (got - want[0][:, y0:y1]).abs().max() <= 1e-12 and (Tg - T[0][:, y0:y1]).abs().max() <= 1e-12, (res_mode, y0, y1)
