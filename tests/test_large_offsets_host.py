"""CPU: the in-image limits tests/test_gpu_large_offsets.py exercises on the GPU, where they can be seen without a launch - a refused
value returns -2 with its message before anything is launched (the pointers below are host memory) -, and the helper that picks which
images of a multi-GiB tensor are checked, and the strip reference of the big-frame cases against the whole-image reference; and of
the cases of tests/test_gpu_large_offsets_scene.py (tests/large_offsets_cases.py) that each crosses what its id names inside its guards."""
import ctypes
import os

import pytest
import torch

import kernel_refs as K
import kt
import large_offsets_cases as LC
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


# ----------------------------------------------------------------------------------------------------------- the scene / loss / tiling cases
# tests/test_gpu_large_offsets_scene.py's cases (tests/large_offsets_cases.py): each crosses what its id names, asks for less than the cap
# and stays inside the guards of its entry point.


def _largest_crosses(tensors, cross):
    got = crossed(max(tensors.values()), 4)
    return cross in got and (cross == "2^31el" or "2^31el" not in got)


def _held(tensors, n=None):
    return 4 * sum(sorted(tensors.values(), reverse=True)[:n]) / LC.GIB


@pytest.mark.parametrize("masks,shape,cross", LC.APPLY_A)
def test_apply_scene_cases(masks, shape, cross):
    c = LC.apply_case(masks, shape, cross)
    assert _largest_crosses(c["tensors"], cross) and LC.gib(c["tensors"]) <= LC.CAP_GIB
    assert 16 <= c["H"] <= LC.SIDE_MAX and 16 <= c["W"] <= LC.SIDE_MAX
    assert c["B"] * c["V"] * -(-c["H"] // 64) * -(-c["W"] // 64) <= 2 ** 31 - 1
    bs = LC.checked_planes((c["B"], c["per"]))
    assert set(boundary_images(c["B"], c["per"], 4)) <= set(bs) and len(bs) >= 5 and bs[-1] == c["B"] - 1 and (c["B"] - 1) * c["per"] >= LC.TOP[cross]        # a whole sample behind the crossing
    if shape == "64x64":            # the control: 2^32 bytes are a whole number of samples, and checked samples lie behind them
        wrap = (1 << 30) // c["per"]
        assert (1 << 30) % c["per"] == 0 and sum(b >= wrap for b in bs) >= 2


@pytest.mark.parametrize("which,shape,cross", LC.BACKWARD_A)
def test_apply_backward_cases(which, shape, cross):
    c = LC.backward_case(which, shape, cross)
    assert _largest_crosses(c["tensors"], cross) and _held(c["tensors"], c["held"]) + 2 <= LC.CAP_GIB
    assert c["B"] * c["V"] * -(-c["H"] // 64) * -(-c["W"] // 64) <= 2 ** 31 - 1 and len(LC.checked_planes((c["B"], c["per"]))) >= 5
    # all five tensors past 2^31 elements would be 40 GiB: why "both" stops past 2^32 bytes
    assert which != "both" or 5 * 4 * (LC.TOP["2^31el"] + c["per"]) / LC.GIB > LC.CAP_GIB


@pytest.mark.parametrize("masks,shape,cross", LC.REDUCE_A)
def test_reduce2_cases(masks, shape, cross):
    c = LC.reduce_case(masks, shape, cross)
    assert _largest_crosses(c["tensors"], cross) and LC.gib(c["tensors"]) <= LC.CAP_GIB
    assert 32 <= c["H"] <= LC.SIDE_MAX and 32 <= c["W"] <= LC.SIDE_MAX
    assert c["N"] * -(-c["H"] // 32) * -(-c["W"] // 128) <= 2 ** 31 - 1                 # reduce2's grid guard (include/hrnet_hip.h)
    assert crossed(c["tensors"]["out"], 4) == (["2^31B"] if shape == "64x64" else [])    # a quarter (or 400 / 1650) of x
    assert len(LC.checked_planes((c["N"], c["H"] * c["W"]), (c["N"], (c["H"] // 2) * (c["W"] // 2)))) >= 5


@pytest.mark.parametrize("shape,border,metric,clip,backward,cross", LC.LOSS_A)
def test_shift_loss_cases(shape, border, metric, clip, backward, cross):
    c = LC.loss_case(shape, border, metric, clip, backward, cross)
    assert _largest_crosses(c["tensors"], cross) and c["B"] <= LC.LOSS_BATCH_MAX and c["B"] % 2 == 0
    assert LC.gib(c["tensors"]) + 1 <= LC.CAP_GIB and border >= 1 and c["H"] * c["W"] <= 2 ** 31 - 1
    assert len(LC.checked_planes((c["B"], c["H"] * c["W"]))) >= 5
    if shape == "128x256":
        wrap = (1 << 30) // (c["H"] * c["W"])
        assert (1 << 30) % (c["H"] * c["W"]) == 0 and sum(b >= wrap for b in boundary_images(c["B"], c["H"] * c["W"], 4)) >= 2
        assert LC.TOP["2^31el"] // (c["H"] * c["W"]) + 2 > LC.LOSS_BATCH_MAX             # why this shape cannot reach 2^31 elements
    if backward:                                                                         # a fourth tensor past 2^31 elements: beyond the cap
        assert 4 * 4 * (LC.TOP["2^31el"] + c["H"] * c["W"]) / LC.GIB + 2 > LC.CAP_GIB


def test_shift_loss_cases_cover_what_the_issue_asks():
    assert any(b == 3 for _, b, *_ in LC.LOSS_A) and any(clip for _, _, _, clip, _, _ in LC.LOSS_A)
    assert any(cross == "2^31el" for *_, cross in LC.LOSS_A) and any(bwd for *_, bwd, _ in LC.LOSS_A)


@pytest.mark.parametrize("path,shape,codes", LC.DIHEDRAL)
def test_dihedral_cases(path, shape, codes):
    c = LC.dihedral_case(path, shape, codes)
    assert len(set(codes)) == c["K"] and (c["K"] - 1) * c["member_elems"] < 1 << 31 < c["K"] * c["member_elems"]
    assert c["member_elems"] >= (1 << 31) // c["K"] and LC.gib(c["tensors"]) <= LC.CAP_GIB
    assert (c["W"] % 4 == 0) == (path == "vec") and (c["H"] == c["W"] or not any(k & 4 for k in codes))
    assert path != "vec" or c["tiles"] <= LC.DIHEDRAL_MAX_TILES
    assert c["K"] < 8 or sorted(codes) == list(range(8))


def test_collate_case():
    L, rows = LC.collate_case()
    assert L % 8 == 0 and crossed(L, 2) == ["2^31B", "2^32B", "2^31el"]
    offs = [o for _, os_, _ in rows for o in os_ if o >= 0]
    v = LC.COLLATE_SIDE ** 2
    for edge in (1 << 30, 1 << 31):                     # an image on either side of byte 2^31 and of byte 2^32
        assert edge in offs and edge - v in offs
    assert 0 in offs and L - v in offs and all(o % 4 == 0 for o in offs)
    (side_g, og, what_g), (side_b, ob, what_b) = rows[-2:]
    assert side_g == side_b == LC.COLLATE_ODD and og[0] + side_g ** 2 == L - 3 and what_g == "good"
    assert ob[0] + side_b ** 2 == L + 1 and what_b == "slot 0 NaN"                       # ONE element past the arena
    for S in LC.COLLATE_S:
        assert all(x + S <= LC.COLLATE_ODD for x in LC.COLLATE_CORNER)
    assert set(LC.COLLATE_CODES) == {0, 3, 5} and [s % 4 == 0 for s in LC.COLLATE_S] == [True, False]


def test_tile_cases(lib):
    from hrnet_hip import tiling
    g, s = LC.gather_case(), LC.scatter_case()
    for c, V in ((g, g["V"]), (s, 9)):
        assert c["R"] == tiling.halo(LC.TILE_LAYERS, V) == lib.hrn_hrnet_halo(LC.TILE_LAYERS, V)
        assert (c["ny"], c["nx"]) == (tiling.axis_count(c["H"], c["t"], c["R"]), tiling.axis_count(c["W"], c["t"], c["R"]))
        assert c["windows"] == lib.hrn_tile_count(c["H"], c["W"], c["t"], c["R"]) and c["rows"] < LC.TILE_MAX_ROWS
        assert c["H"] % 64 and c["W"] % 64 and c["H"] != c["W"]
    assert g["H"] <= LC.SIDE_MAX and g["W"] <= LC.SIDE_MAX and g["H"] * g["W"] <= 2 ** 31 - 1
    assert all("2^31el" in crossed(n, 4) for n in g["tensors"].values()) and LC.gib(g["tensors"]) <= LC.CAP_GIB
    out = s["tensors"]["out"]
    assert out <= 2 ** 31 - 1 and crossed(out, 4) == ["2^31B", "2^32B"] and "2^31el" in crossed(s["tensors"]["srs"], 4)
    assert LC.gib(s["tensors"]) <= LC.CAP_GIB
    # the row of windows that is left out holds no crossing of either tensor
    a, b = s["skip"]
    St = s["S"] * s["t"]
    plan = tiling.plan(s["H"], s["W"], s["t"], s["R"])
    rows = {w.y0 for w in plan.windows[a:b]}
    assert b - a == s["nx"] and len(rows) == 1
    lo, hi = s["S"] * min(w.y0 for w in plan.windows[a:b]), s["S"] * (max(w.y0 for w in plan.windows[a:b]) + s["t"])
    for e in crossings(out, 4):
        assert not lo <= e // (s["S"] * s["W"]) < hi
    for e in crossings(s["tensors"]["srs"], 4):
        assert not a <= e // (St * St) < b


def test_the_smallest_refused_shapes(lib):
    """hrn_tile_scatter and hrn_shift_cssim refuse the first square past their in-plane limit (and the square before it is inside it):
    -2 with the message, before anything is launched (the pointers are host memory)"""
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    H, W, S = (LC.SCATTER_REFUSED[k] for k in ("H", "W", "S"))
    assert S * S * (H - 1) * (W - 1) <= 2 ** 31 - 1 < S * S * H * W and H * W <= 2 ** 31 - 1
    rc = lib.hrn_tile_scatter(p, 1, H, W, 128, 15, S, 0, 1, p, None)
    assert rc == -2 and f"the x{S} plane of H={H} x W={W} is beyond 32-bit in-plane offsets".encode() in lib.hrn_last_error()
    H, W = LC.CSSIM_REFUSED["H"], LC.CSSIM_REFUSED["W"]
    assert (H - 1) * (W - 1) <= 2 ** 31 - 1 < H * W
    rc = lib.hrn_shift_cssim(p, p, p, 1, H, W, 1, 1, 0, 1, 1.0, p, p, p, p, 1 << 62, None)
    assert rc == -2 and f"cssim: a frame of {H} x {W} exceeds 2^31 pixels".encode() in lib.hrn_last_error()


@pytest.mark.parametrize("kind,shape,border,option,clip,backward,cross", LC.SEARCHED_A)
def test_searched_loss_cases(lib, kind, shape, border, option, clip, backward, cross):
    c = LC.searched_case(kind, shape, border, option, clip, backward, cross)
    B, H, W = c["B"], c["H"], c["W"]
    assert _largest_crosses(c["tensors"], cross) and B <= LC.LOSS_BATCH_MAX and B % 2 == 0 and H * W <= 2 ** 31 - 1
    assert len(LC.checked_planes((B, H * W))) >= 5 and all(0 <= p <= 2 * border for p in LC.PLANT) and border >= 1
    if kind == "cl1":
        ws = lib.hrn_cl1_loss_workspace_bytes(B, H, W, border)
    else:
        ws = max(lib.hrn_shift_cssim_workspace_bytes(B, H, W, border, option), lib.hrn_cssim_loss_backward_workspace_bytes(B, H, W, border, option))
    assert ws > 0 and LC.gib(c["tensors"], ws) <= LC.CAP_GIB          # the workspace from the size query is part of what the case asks for
    # the shift-searched loss's own cases, with their workspace
    for case in LC.LOSS_A:
        s = LC.loss_case(*case)
        assert LC.gib(s["tensors"], lib.hrn_shift_loss_workspace_bytes(s["B"], s["H"], s["W"], s["border"])) <= LC.CAP_GIB


def test_searched_loss_cases_cover_what_the_issue_asks():
    for kind in ("cl1", "cssim"):
        mine = [c for c in LC.SEARCHED_A if c[0] == kind]
        assert any(c[2] == 3 for c in mine) and any(c[4] for c in mine) and any(c[5] for c in mine) and any(c[6] == "2^31el" for c in mine)
        assert len({c[3] for c in mine}) == 2                           # both eps / both windows


@pytest.mark.parametrize("which,shape,cross", LC.LANCZOS_A)
def test_lanczos_cases(lib, which, shape, cross):
    c = LC.lanczos_case(which, shape, cross)
    assert _largest_crosses(c["tensors"], cross) and c["c"] <= 65535 and len(LC.checked_planes((c["c"], c["H"] * c["W"]))) >= 5
    ws = lib.hrn_lanczos_shift_backward_workspace_bytes(1, c["c"], c["H"], c["W"]) if which == "bwd" else 0
    assert LC.gib(c["tensors"], ws) <= LC.CAP_GIB
    if which == "bwd":              # past 2^31 elements the three tensors and the workspace would be beyond the cap
        big = LC.lanczos_case(which, shape, "2^31el")
        assert LC.gib(big["tensors"], lib.hrn_lanczos_shift_backward_workspace_bytes(1, big["c"], big["H"], big["W"])) > LC.CAP_GIB


@pytest.mark.parametrize("masks,shape,cross", LC.SEARCH_A)
def test_search_scene_cases(lib, masks, shape, cross):
    c = LC.search_case(masks, shape, cross)
    B, V, H, W = c["B"], c["V"], c["H"], c["W"]
    ws = lib.hrn_mncc_scene_workspace_bytes(B, V, H, W, LC.MNCC_P)
    assert _largest_crosses(c["tensors"], cross) and ws > 0 and LC.gib(c["tensors"], ws) <= LC.CAP_GIB
    assert 16 <= H <= LC.SIDE_MAX and 16 <= W <= LC.SIDE_MAX and c["tiles"] <= 2 ** 31 - 1 and V == 2
    assert lib.hrn_mncc_scene_workspace_bytes(B, V, H, W, LC.MNCC_P - 1) == 0           # P is the smallest the entry points take
    views, ref = set(boundary_images(B, c["per"], 4)), set(boundary_images(B, H * W, 4))
    # with V = 2 the reference's byte crossings fall on the samples of the views' next crossings: the union is checked all the same
    assert set(LC.checked_planes((B, c["per"]), (B, H * W))) >= views | ref


@pytest.mark.parametrize("masks,shape,cross", LC.LOCAL_A)
def test_search_local_cases(lib, masks, shape, cross):
    c = LC.local_case(masks, shape, cross)
    B, V, H, W = c["B"], c["V"], c["H"], c["W"]
    ws = lib.hrn_mncc_local_workspace_bytes(B, V, H, W, LC.MNCC_P, LC.LOCAL_BLOCK)
    assert _largest_crosses(c["tensors"], cross) and ws > 0 and LC.gib(c["tensors"], ws) <= LC.CAP_GIB
    assert LC.gib({**c["search"], "views": c["tensors"]["views"], "view_masks": c["tensors"].get("view_masks", 0)}, ws) <= LC.CAP_GIB
    assert (c["by"], c["bx"]) == (lib.hrn_mncc_local_blocks(H, LC.LOCAL_BLOCK), lib.hrn_mncc_local_blocks(W, LC.LOCAL_BLOCK))
    assert lib.hrn_mncc_local_blocks(H, LC.LOCAL_BLOCK - 64) == 0 and c["tiles"] <= 2 ** 31 - 1 and B * V * c["by"] * c["bx"] <= 2 ** 31 - 1
    assert shape == "64x64" or (c["by"] >= 2 and c["bx"] >= 2 and H % 64 and W % 64)
    assert len(LC.checked_planes((B, c["per"]), (B, H * W))) >= 5


@pytest.mark.parametrize("masks,V,cross", LC.FRAME_B)
def test_big_frame_cases(lib, masks, V, cross):
    c = LC.frame_case(masks, V, cross)
    H, W = c["H"], c["W"]
    assert _largest_crosses(c["tensors"], cross) and LC.gib(c["tensors"]) <= LC.CAP_GIB
    assert H <= LC.SIDE_MAX and W <= LC.SIDE_MAX and H % 64 and W % 64 and H != W
    assert V * -(-H // 64) * -(-W // 64) <= 2 ** 31 - 1 and V * -(-H // 32) * -(-W // 128) <= 2 ** 31 - 1
    assert (c["by"], c["bx"]) == (lib.hrn_mncc_local_blocks(H, LC.FRAME_BLOCK), lib.hrn_mncc_local_blocks(W, LC.FRAME_BLOCK)) and c["by"] >= 2
    strips = LC.frame_strips(V, H, W)
    assert len(strips) >= 5 and all(0 <= y0 < y1 <= H and y1 - y0 >= 24 and y0 % 2 == 0 and 0 <= p < V for p, y0, y1 in strips)
    for e in crossings(V * H * W, 4):           # every crossing lies inside a checked strip
        assert any(p * H * W + y0 * W <= e < p * H * W + y1 * W for p, y0, y1 in strips)
    assert {p for p, _, _ in strips} >= {0, V - 1}


def test_strip_restatements_are_the_whole_frame_restatements():
    """At a small size: the restatement of a strip with its real neighbour rows, as tests/test_gpu_large_offsets_scene.py runs it on the
    big frames, equals the whole-frame restatement on the strip's rows - the sampler and its valid map, d_views, reduce2 and the field
    sampler"""
    import numpy as np
    import registration_local_ref as L
    import registration_pyramid_ref as Y
    import registration_ref as R
    import warp_ref as WR
    H, W, block = 150, 61, 64
    rng = np.random.default_rng(3)
    T, M = rng.random((H, W)).astype(np.float32), (rng.random((H, W)) > 0.15).astype(np.float32)
    g = rng.standard_normal((H, W)).astype(np.float32)
    field = (rng.uniform(-2.5, 2.5, (L.blocks(H, block), L.blocks(W, block), 2)) + 0.013).astype(np.float32)
    px_all = L.field_at_pixels(field, H, W, block)
    f_all = L.sample_field(T, M, px_all)
    r_all = Y.reduce2(T, M)
    for y0, y1 in ((0, 24), (62, 86), (H - 24, H)):
        for s in WR.SHIFTS[:6]:
            s = np.array(s, np.float32)
            ny = abs(R.split(s[0])[0])
            a, b = LC.with_reach(H, y0, y1, ny + 4)
            sl = slice(y0 - a, y1 - a)
            assert np.array_equal(R.sample(T[a:b], s)[sl], R.sample(T, s)[y0:y1]) and np.array_equal(R.shifted_mask(M[a:b], s)[sl], R.shifted_mask(M, s)[y0:y1])
            k = R.shifted_mask(M, s).astype(np.float32)
            a, b = LC.with_reach(H, y0, y1, 2 * (ny + 4))
            sl = slice(y0 - a, y1 - a)
            assert np.abs(WR.d_views(g[a:b], k[a:b], s)[sl] - WR.d_views(g, k, s)[y0:y1]).max() <= 1e-15
            assert np.abs(WR.magnitudes(np.zeros_like(g[a:b]), g[a:b], k[a:b], s)[0][sl] - WR.magnitudes(T, g, k, s)[0][y0:y1]).max() <= 1e-15
        a, b = LC.with_reach(H, y0, y1, 8)
        sl = slice(y0 - a, y1 - a)
        px = L.field_at_pixels(field, H, W, block, rows=(a, b))
        assert np.array_equal(px, px_all[a:b])
        for part, whole in zip(L.sample_field(T[a:b], M[a:b], px), f_all):
            assert np.array_equal(part[sl], whole[y0:y1])
        Y0, Y1 = y0 // 2, min(H // 2, y1 // 2)
        a, b = max(0, 2 * Y0 - 2), min(H, 2 * Y1 + 2)
        for part, whole in zip(Y.reduce2(T[a:b], M[a:b]), r_all):
            assert np.array_equal(part[Y0 - a // 2:Y1 - a // 2], whole[Y0:Y1])


def test_lanczos_big_frame_case_and_its_strip_restatement(lib):
    import kernel_refs as K
    H, W, reach = LC.LANCZOS_B["H"], LC.LANCZOS_B["W"], LC.LANCZOS_B["reach"]
    assert crossed(H * W, 4) == ["2^31B", "2^32B"] and H % 64 and W % 64
    assert LC.gib({k: H * W for k in "abc"}, lib.hrn_lanczos_shift_backward_workspace_bytes(1, 1, H, W)) <= LC.CAP_GIB
    assert LC.gib({k: 1 << 31 for k in "abc"}, 8 << 30) > LC.CAP_GIB                     # why not 2^31 elements in one plane
    strips = LC.frame_strips(1, H, W)
    assert len(strips) >= 5 and strips[0][1] == 0 and max(y1 for _, _, y1 in strips) == H
    # at a small size: the strip with four neighbour rows against the whole plane, forward and d_img
    g = torch.Generator().manual_seed(5)
    h, w = 90, 37
    img, dout = torch.rand((1, 1, h, w), generator=g, dtype=torch.float64), torch.randn((1, 1, h, w), generator=g, dtype=torch.float64)
    s = K.TAIL_SHIFTS[2:3].double()
    whole = (K.ref_lanczos_shift(img, s), K.lanczos_shift_T(img, s), K.ref_lanczos_grads(torch.zeros_like(img), s, dout)[0], K.lanczos_dimg_T(dout, s))
    for y0, y1 in ((0, 24), (30, 54), (h - 24, h)):
        a, b = LC.with_reach(h, y0, y1, reach)
        sl = slice(y0 - a, y1 - a)
        x, d = img[:, :, a:b], dout[:, :, a:b]
        part = (K.ref_lanczos_shift(x, s), K.lanczos_shift_T(x, s), K.ref_lanczos_grads(torch.zeros_like(x), s, d)[0], K.lanczos_dimg_T(d, s))
        for p, q in zip(part, whole):
            assert (p[:, :, sl] - q[:, :, y0:y1]).abs().max() <= 1e-14


@pytest.mark.parametrize("kind,H,W,option,backward,cross", LC.LOSS_B)
def test_losses_big_frame_cases(lib, kind, H, W, option, backward, cross):
    b = LC.LOSS_B_BORDER
    ws = {"shift": lambda: lib.hrn_shift_loss_workspace_bytes(1, H, W, b), "cl1": lambda: lib.hrn_cl1_loss_workspace_bytes(1, H, W, b),
          "cssim": lambda: max(lib.hrn_shift_cssim_workspace_bytes(1, H, W, b, option), lib.hrn_cssim_loss_backward_workspace_bytes(1, H, W, b, option))}[kind]()
    assert ws > 0 and LC.gib({k: H * W for k in range(4 if backward else 3)}, ws) <= LC.CAP_GIB and H * W <= 2 ** 31 - 1
    strips = LC.loss_b_strips(H, W)
    if cross == "2^32B":
        assert crossed(H * W, 4) == ["2^31B", "2^32B"] and len(strips) >= 5 and sum(y1 * W > 1 << 30 for _, y1 in strips) >= 2
    else:       # the int limit of cssim.hip: the last strip's pixels, plus an offset of up to 2 border rows, reach within 2 W of 2^31
        assert (H + 1) * (W + 1) > 2 ** 31 - 1 and strips[-1] == (H - 64, H) and H * W + 2 * W > 1 << 31 and len(strips) == 2
    reach = 2 * b + max(LC.CSSIM_TAPS.values())
    assert all(y1 + reach <= y0 - reach for (_, y1), (y0, _) in zip(strips, strips[1:]))


def test_the_stacked_strips_give_the_whole_frames_losses():
    """shift_loss_ref.frame_of_row_ranges at a small size, the map clear only in three strips: the stacked frame's cMSE / cPSNR, cL1 and
    their gradients are the whole frame's; cSSIM's scores and gradient after the scaling by the map pixels"""
    import cl1_ref
    import cssim_grad_ref as G
    import cssim_ref as CR
    import numpy as np
    import shift_loss_ref as R
    H, W, b = 160, 40, 1
    g = torch.Generator().manual_seed(9)
    srs = torch.rand((H, W), generator=g)
    hrs = torch.roll(srs, (-1, 1), (0, 1)) + 0.05 * torch.randn((H, W), generator=g)
    strips = [(0, 12), (70, 90), (H - 16, H)]
    maps = torch.zeros((H, W))
    for y0, y1 in strips:
        maps[y0:y1] = (torch.rand((y1 - y0, W), generator=g) > 0.1).float()
    rows_of = lambda a, c: (srs[a:c], hrs[a:c], maps[a:c])
    for kind, T in (("shift", 1), ("cl1", 1), ("cssim", 7)):
        small, windows = R.frame_of_row_ranges(rows_of, strips, H, 2 * b + T)
        assert small[0].shape[1] < H and windows[0][0] == 0 and windows[-1][1] == H
        rows = np.concatenate([np.arange(a, c) for a, c in windows])
        if kind == "cssim":
            scale = (small[0].shape[1] - 2 * b - T + 1) / (H - 2 * b - T + 1)
            whole = CR.shift_cssim(srs.numpy(), hrs.numpy(), maps.numpy(), b, "uniform", False, True, 1.0)
            part = CR.shift_cssim(*(t[0].numpy() for t in small), b, "uniform", False, True, 1.0)
            assert whole[1] == part[1] and np.abs(1.0 + (part[0] - 1.0) * scale - whole[0]).max() <= 1e-12
            gw = G.grad(srs.numpy(), hrs.numpy(), maps.numpy(), whole[1], b, "uniform", False, True, 1.0)
            gp = G.grad(*(t[0].numpy() for t in small), part[1], b, "uniform", False, True, 1.0) * scale
        else:
            fn = (lambda s, h, m: R.shift_loss(s, h, m, "cPSNR", b, False)) if kind == "shift" else (lambda s, h, m: cl1_ref.cl1_loss(s, h, m, b, False, 1e-3))
            res = []
            for s, h, m in ((srs[None], hrs[None], maps[None]), small):
                s = s.double().requires_grad_(True)
                out = fn(s, h, m)
                out[0].sum().backward()
                res.append((float(out[0].detach()), int(out[1][0]), s.grad[0].numpy()))
            assert res[0][1] == res[1][1] and abs(res[0][0] - res[1][0]) <= 1e-12 * abs(res[0][0])
            gw, gp = res[0][2], res[1][2]
        assert np.abs(gw[rows] - gp).max() <= 1e-12 * np.abs(gw).max() and np.count_nonzero(np.delete(gw, rows, 0)) == 0 and np.abs(gw).max() > 0


@pytest.mark.parametrize("masks,V,cross", LC.FRAME_B)
def test_sum_blocks_and_their_stacked_restatement(masks, V, cross):
    """the blocks of test_scene_sums_big_frame hold the row of every crossing of the view stack and keep SUM_INSET from the frame's edges;
    at a small size, the scores and d_shifts of a frame whose gating mask is clear only in such blocks are those of the stacked windows"""
    import numpy as np
    import registration_ref as R
    import warp_ref as WR
    H, W = LC.FRAME_H, LC.FRAME_W
    blocks = LC.sum_blocks(V, H, W)
    assert len(blocks) >= 5 and all(LC.SUM_INSET <= y0 < y1 <= H - LC.SUM_INSET and LC.SUM_INSET <= x0 < x1 <= W - LC.SUM_INSET for y0, y1, x0, x1 in blocks)
    assert len({x1 - x0 for _, _, x0, x1 in blocks}) == 1
    for e in crossings(V * H * W, 4):
        r = (e % (H * W)) // W
        assert any(y0 <= r < y1 for y0, y1, _, _ in blocks)
    assert max(abs(R.split(np.float32(d))[0]) for s in WR.SHIFTS[:5] for d in s) + 3 <= LC.SUM_REACH
    # small: a 120 x 150 frame, blocks of 10 x 20
    h, w, r = 120, 150, LC.SUM_REACH
    small = [(y0, y0 + 10, x0, x0 + 20) for y0 in (16, 60, 94) for x0 in (16, 70, 114)]
    rng = np.random.default_rng(11)
    view = rng.random((h, w)).astype(np.float32)
    ref = (view + 0.1 * rng.standard_normal((h, w))).astype(np.float32)
    vm = (rng.random((h, w)) > 0.15).astype(np.float32)
    gate = np.zeros((h, w), np.float32)
    for y0, y1, x0, x1 in small:
        gate[y0:y1, x0:x1] = rng.random((y1 - y0, x1 - x0)) > 0.15
    stack = lambda t: np.concatenate([t[y0 - r:y1 + r, x0 - r:x1 + r] for y0, y1, x0, x1 in small])
    for centre in ((0.0, 0.0), (-1.3, 0.7), (1.75, -0.5)):
        whole = R.grid(ref, gate, view, vm, np.float32(centre), np.float32(2.0), 3)[0]
        part = R.grid(stack(ref), stack(gate), stack(view), stack(vm), np.float32(centre), np.float32(2.0), 3)[0]
        assert np.isfinite(whole).all() and np.abs(whole - part).max() <= 1e-12
    g = rng.standard_normal((h, w)).astype(np.float32)
    for s in WR.SHIFTS[:5]:
        s = np.array(s, np.float32)
        whole, part = WR.d_shifts(view, g, gate, s), WR.d_shifts(stack(view), stack(g), stack(gate), s)
        assert np.abs(whole - part).max() <= 1e-12 * np.abs(whole).max() and np.abs(whole).max() > 0
        assert np.abs(WR.magnitudes(view, g, gate, s)[1] - WR.magnitudes(stack(view), stack(g), stack(gate), s)[1]).max() <= 1e-9
